"""ctypes binding of polaris_amd/lib/libpolaris_host.so: the C++ host layer (tracer.Tracer mirror,
Naive/Perfect schedulers of tracer/scheduler.go, frame loop of renderer/default.go)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import ctypes_api as T

LIB_PATH = os.path.join(T.LIB_DIR, "libpolaris_host.so")
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        T.load_library()  # dependency first (same directory, rpath $ORIGIN)
        lib = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        lib.polaris_host_scheduler_new.restype = vp
        lib.polaris_host_scheduler_new.argtypes = [C.c_int, vp, C.c_uint32]
        lib.polaris_host_scheduler_schedule.argtypes = [vp, vp, vp, C.c_uint32, vp]
        lib.polaris_host_scheduler_schedule.restype = None
        lib.polaris_host_scheduler_free.argtypes = [vp]
        lib.polaris_host_scheduler_free.restype = None
        lib.polaris_host_renderer_new.restype = vp
        lib.polaris_host_renderer_new.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(T.SceneView), vp, vp, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_char_p]
        lib.polaris_host_renderer_render.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_double)]
        lib.polaris_host_renderer_push_seeds.argtypes = [vp, C.c_uint32, vp, C.c_size_t]
        lib.polaris_host_renderer_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        lib.polaris_host_renderer_set_denoise.argtypes = [vp, C.POINTER(T.DenoiseParams)]
        lib.polaris_host_renderer_update_instances.argtypes = [vp, C.POINTER(T.InstanceUpdate)]
        lib.polaris_host_renderer_update_vertices.argtypes = [vp, C.POINTER(T.VertexUpdate)]
        lib.polaris_host_renderer_update_materials.argtypes = [vp, C.POINTER(T.MaterialUpdate)]
        lib.polaris_host_renderer_update_texture.argtypes = [vp, C.c_uint32, vp, C.c_size_t]
        lib.polaris_host_renderer_upload_scene.argtypes = [vp, C.POINTER(T.SceneView)]
        lib.polaris_host_renderer_read_aov.argtypes = [vp, C.c_int, vp, C.c_size_t]
        lib.polaris_host_renderer_set_temporal.argtypes = [vp, C.POINTER(T.TemporalParams)]
        lib.polaris_host_renderer_set_camera.argtypes = [vp, vp, vp]
        lib.polaris_host_renderer_set_lens.argtypes = [vp, C.c_float, C.c_float]
        lib.polaris_host_renderer_set_shutter.argtypes = [vp, vp, vp, C.c_float]
        lib.polaris_host_renderer_set_projection.argtypes = [vp, C.c_uint32, C.c_float, C.c_float, C.c_float]
        lib.polaris_host_renderer_set_variance.argtypes = [vp, C.POINTER(T.VarianceParams)]
        lib.polaris_host_renderer_set_display.argtypes = [vp, C.POINTER(T.DisplayParams)]
        lib.polaris_host_renderer_read_exposure.argtypes = [vp, C.POINTER(T.ExposureInfo), vp]
        lib.polaris_host_renderer_set_bloom.argtypes = [vp, C.POINTER(T.BloomParams)]
        u32 = C.c_uint32
        lib.polaris_host_bloom.argtypes = [vp, u32, u32, u32, u32, C.c_float, C.c_float, C.POINTER(T.DisplayParams), C.POINTER(T.BloomParams),
                                           C.POINTER(C.c_float), vp, vp, vp, C.POINTER(u32)]
        lib.polaris_host_bloom_check.argtypes = [C.POINTER(T.BloomParams)]
        lib.polaris_host_bloom_levels.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
        lib.polaris_host_bloom_levels.restype = u32
        lib.polaris_host_display.argtypes = [vp, u32, u32, u32, u32, C.c_float, C.c_float, C.POINTER(T.DisplayParams), C.POINTER(C.c_float), vp, vp,
                                             C.POINTER(T.ExposureInfo)]
        lib.polaris_host_variance.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, C.POINTER(T.DenoiseParams), C.POINTER(T.VarianceParams), vp]
        lib.polaris_host_denoise_variance.argtypes = [vp, C.c_float, vp, vp, vp, u32, u32, u32, u32, C.POINTER(T.DenoiseParams),
                                                      C.POINTER(T.VarianceParams), vp]
        lib.polaris_host_reproject_moments.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, C.POINTER(T.TemporalParams), vp, vp]
        lib.polaris_host_reproject.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(T.TemporalParams), vp]
        lib.polaris_host_reproject_motion.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, C.POINTER(T.TemporalParams),
                                                      vp, vp, vp]
        lib.polaris_host_reproject_deform.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, C.POINTER(T.TemporalParams),
                                                      vp, vp, vp, vp, vp, vp, u32]
        lib.polaris_host_motion_matrix.argtypes = [vp, vp, C.POINTER(u32), vp]
        lib.polaris_host_reproject_projection.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(T.ProjectionParams), u32, u32, C.POINTER(T.TemporalParams), vp]
        lib.polaris_host_projection_rays.argtypes = [C.POINTER(T.ProjectionParams), vp, u32, u32, vp, vp]
        lib.polaris_host_projection_project.argtypes = [C.POINTER(T.ProjectionParams), vp, vp, u32, vp, vp]
        lib.polaris_host_temporal_combine.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        lib.polaris_host_camera_move.argtypes = [vp, C.c_float, C.c_int, vp, vp, C.c_uint32, vp, vp, vp]
        lib.polaris_host_denoise.argtypes = [vp, C.c_float, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.POINTER(T.DenoiseParams), vp]
        lib.polaris_host_renderer_read.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
        lib.polaris_host_renderer_merge_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
        lib.polaris_host_renderer_tracer_stats.argtypes = [vp, C.c_uint32, C.POINTER(T.TraceStats), C.POINTER(C.c_double)]
        lib.polaris_host_renderer_save.argtypes = [vp, C.c_char_p]
        lib.polaris_host_write_png.argtypes = [C.c_char_p, vp, C.c_uint32, C.c_uint32]
        lib.polaris_host_renderer_error.argtypes = [vp]
        lib.polaris_host_renderer_error.restype = C.c_char_p
        lib.polaris_host_renderer_free.argtypes = [vp]
        lib.polaris_host_renderer_free.restype = None
        lib.polaris_host_bvh_build.restype = C.c_uint32
        lib.polaris_host_bvh_build.argtypes = [vp, C.c_uint32, C.c_int, vp, C.c_uint32, vp, vp]
        lib.polaris_host_compile_scene.restype = vp
        lib.polaris_host_compile_scene.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp,
                                                   C.c_uint32, vp, C.c_uint32, C.c_int32, C.c_int32, C.c_int, C.c_char_p]
        lib.polaris_host_compiled_view.restype = C.POINTER(T.SceneView)
        lib.polaris_host_compiled_view.argtypes = [vp]
        lib.polaris_host_compiled_free.argtypes = [vp]
        lib.polaris_host_compiled_free.restype = None
        lib.polaris_host_material_check.argtypes = [C.c_char_p, C.c_char_p]
        lib.polaris_host_material_ior.argtypes = [C.c_char_p, C.POINTER(C.c_float)]
        lib.polaris_host_read_scene.restype = vp
        lib.polaris_host_read_scene.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
        lib.polaris_host_compiled_camera.argtypes = [vp, C.c_float, C.c_int, vp, vp, vp]
        lib.polaris_host_compiled_camera.restype = None
        lib.polaris_host_compiled_warnings.argtypes = [vp, C.c_char_p, C.c_size_t]
        lib.polaris_host_compiled_warnings.restype = C.c_size_t
        lib.polaris_host_parse_obj.argtypes = [C.c_char_p, vp, vp, vp, C.c_uint32, C.c_char_p, C.c_size_t, C.c_char_p]
        lib.polaris_host_parse_mtl.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p]
        lib.polaris_host_select_face_index.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p]
        lib.polaris_host_texture_load.argtypes = [C.c_char_p, vp, vp, C.c_size_t, C.c_char_p]
        _lib = lib
    return _lib


NAIVE, PERFECT = 0, 1


class Scheduler:
    """tracer.NaiveScheduler() / tracer.PerfectScheduler() over mock tracers with the given speeds."""

    def __init__(self, kind: int, speeds):
        self._lib = load()
        self._speeds = np.ascontiguousarray(speeds, dtype=np.uint32)
        self._h = self._lib.polaris_host_scheduler_new(kind, self._speeds.ctypes.data, len(self._speeds))

    def schedule(self, frame_h: int, block_h=None, render_ns=None) -> list[int]:
        n = len(self._speeds)
        out = np.zeros(n, dtype=np.uint32)
        bh = None if block_h is None else np.ascontiguousarray(block_h, dtype=np.uint32)
        rt = None if render_ns is None else np.ascontiguousarray(render_ns, dtype=np.int64)
        self._lib.polaris_host_scheduler_schedule(self._h, None if bh is None else bh.ctypes.data, None if rt is None else rt.ctypes.data,
                                                  frame_h, out.ctypes.data)
        return [int(v) for v in out]

    def close(self):
        if self._h:
            self._lib.polaris_host_scheduler_free(self._h)
            self._h = None

    __del__ = close


class Renderer:
    """renderer.NewDefault over HipTracers (device_indices may repeat one GPU)."""

    def __init__(self, scene, device_indices, *, primary=0, scheduler=NAIVE, width=64, height=64, spp=4, bounces=5, min_rr=3,
                 exposure=1.2, seed=1):
        self._lib = load()
        self._scene = scene
        self._view = T.scene_view(scene)
        self.W, self.H, self.n = width, height, len(device_indices)
        dev = np.ascontiguousarray(device_indices, dtype=np.int32)
        eye = np.ascontiguousarray(scene.eye, dtype=np.float32)
        fr = np.ascontiguousarray(scene.frustum, dtype=np.float32)
        err = C.create_string_buffer(256)
        self._h = self._lib.polaris_host_renderer_new(dev.ctypes.data, self.n, primary, scheduler, C.byref(self._view), eye.ctypes.data,
                                                      fr.ctypes.data, width, height, spp, bounces, min_rr, exposure, seed, err)
        if not self._h:
            raise RuntimeError(f"renderer: {err.value.decode()}")

    def push_seeds(self, tracer_index: int, seeds) -> None:
        """Test hook: tracer `tracer_index` takes its next host PRNG draws (one per sample + one per bounce,
        tracer.go:222, pipeline.go:146) from this list."""
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        if self._lib.polaris_host_renderer_push_seeds(self._h, tracer_index, s.ctypes.data, s.size):
            raise RuntimeError("push_seeds: bad tracer index")

    def set_option(self, key: str, value: int) -> None:
        if self._lib.polaris_host_renderer_set_option(self._h, key.encode(), int(value)):
            raise RuntimeError(f"set_option failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_denoise(self, iterations: int = 4, normal_power_log2: int = 5, sigma_depth: float = 0.1, sigma_luminance: float = 4.0) -> None:
        """polaris_hip_set_denoise on every tracer; only the primary syncs, so only the primary filters."""
        p = T.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_luminance)
        if self._lib.polaris_host_renderer_set_denoise(self._h, C.byref(p)):
            raise RuntimeError(f"set_denoise failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_temporal(self, max_history: int = 32, normal_threshold: float = 0.9, depth_threshold: float = 0.1) -> None:
        """polaris_hip_set_temporal on every tracer; only the primary syncs, so only the primary reprojects."""
        p = T.temporal_params(max_history, normal_threshold, depth_threshold)
        if self._lib.polaris_host_renderer_set_temporal(self._h, C.byref(p)):
            raise RuntimeError(f"set_temporal failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_object_motion(self, on: bool = True) -> None:
        """The option "object_motion" on every tracer (temporal reuse across moving mesh instances); only the primary syncs,
        so only the primary's history is ever used."""
        self.set_option("object_motion", 1 if on else 0)

    def upload_scene(self, scene) -> None:
        """A new scene: UpdateState(SceneData) on every tracer.  Options that apply to the next upload ("instance_update") take
        effect here; the constructor's upload came before any option."""
        self._scene, self._view = scene, T.scene_view(scene)
        if self._lib.polaris_host_renderer_upload_scene(self._h, C.byref(self._view)):
            raise RuntimeError(f"upload_scene failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def update_instances(self, inv, boxes, emissives=None) -> None:
        """polaris_hip_update_instances on every tracer: move the scene's mesh instances in place.  Arguments as
        HipTracer.update_instances; the scene must have been uploaded with the option on: set_option("instance_update", 1), then
        upload_scene (the constructor's upload came before any option)."""
        u, keep = T.instance_update(inv, boxes, emissives)
        if self._lib.polaris_host_renderer_update_instances(self._h, C.byref(u)):
            raise RuntimeError(f"update_instances failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")
        del keep

    def update_vertices(self, vertices, boxes, normals=None, inv=None, emissives=None) -> None:
        """polaris_hip_update_vertices on every tracer: deform the scene's meshes in place.  Arguments as
        HipTracer.update_vertices; the scene must have been uploaded with the option on: set_option("vertex_update", 1), then
        upload_scene (the constructor's upload came before any option)."""
        u, keep = T.vertex_update(vertices, boxes, normals, inv, emissives)
        if self._lib.polaris_host_renderer_update_vertices(self._h, C.byref(u)):
            raise RuntimeError(f"update_vertices failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")
        del keep

    def update_materials(self, nodes, material_index=None, scene_diffuse=-1, emissive_mat_nodes=None) -> None:
        """polaris_hip_update_materials on every tracer: edit the scene's materials in place.  Arguments as
        HipTracer.update_materials; no upload option."""
        u, keep = T.material_update(nodes, material_index, scene_diffuse, emissive_mat_nodes)
        if self._lib.polaris_host_renderer_update_materials(self._h, C.byref(u)):
            raise RuntimeError(f"update_materials failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")
        del keep

    def update_texture(self, index: int, texels) -> None:
        """polaris_hip_update_texture on every tracer: the texels of one texture, same format and size as uploaded."""
        t = np.ascontiguousarray(texels)
        if self._lib.polaris_host_renderer_update_texture(self._h, int(index), t.ctypes.data, t.nbytes):
            raise RuntimeError(f"update_texture failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_variance(self, sigma_variance: float = 8.0, min_samples: int = 8) -> None:
        """polaris_hip_set_variance on every tracer, after the option "moments" on every tracer (polaris_host_renderer_set_variance)."""
        p = T.variance_params(sigma_variance, min_samples)
        if self._lib.polaris_host_renderer_set_variance(self._h, C.byref(p)):
            raise RuntimeError(f"set_variance failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_display(self, enabled: int = 1, **fields) -> None:
        """polaris_hip_set_display on every tracer (polaris_host_renderer_set_display): the display transform of the primary's
        SyncFramebuffer.  fields: those of ctypes_api.DISPLAY_DEFAULTS; enabled = 0 turns it off."""
        p = T.display_params(enabled, **fields)
        if self._lib.polaris_host_renderer_set_display(self._h, C.byref(p)):
            raise RuntimeError(f"set_display failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_bloom(self, enabled: int = 1, **fields) -> None:
        """polaris_hip_set_bloom on every tracer (polaris_host_renderer_set_bloom): the bloom of the primary's displayed SyncFramebuffer,
        in effect while set_display is on.  fields: those of ctypes_api.BLOOM_DEFAULTS; enabled = 0 turns it off."""
        p = T.bloom_params(enabled, **fields)
        if self._lib.polaris_host_renderer_set_bloom(self._h, C.byref(p)):
            raise RuntimeError(f"set_bloom failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def read_exposure(self) -> dict:
        """polaris_hip_read_exposure of the primary: what its last sync with auto-exposure on metered, as display()'s info, with the
        256 counts under "histogram"."""
        info, hist = T.ExposureInfo(), np.zeros(256, np.uint32)
        if self._lib.polaris_host_renderer_read_exposure(self._h, C.byref(info), hist.ctypes.data):
            raise RuntimeError(f"read_exposure failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")
        return dict(exposure_info(info), histogram=hist)

    def set_camera(self, eye, frustum) -> None:
        """A camera move: UpdateState(CameraData) on every tracer (DefaultRenderer::UpdateAll)."""
        e = np.ascontiguousarray(eye, dtype=np.float32).reshape(3)
        f = np.ascontiguousarray(frustum, dtype=np.float32).reshape(16)
        if self._lib.polaris_host_renderer_set_camera(self._h, e.ctypes.data, f.ctypes.data):
            raise RuntimeError(f"set_camera failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_lens(self, radius: float, focus_distance: float = 0.0) -> None:
        """The thin lens on every tracer (CameraData.lens_radius / focus_distance: each tracer's UpdateState(CameraData) sets the lens
        after the camera, from the frustum); later set_camera calls keep it.  radius = 0 turns it off."""
        if self._lib.polaris_host_renderer_set_lens(self._h, float(radius), float(focus_distance)):
            raise RuntimeError(f"set_lens failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_shutter(self, eye_close, frustum_close=None, focus_close: float | None = None) -> None:
        """The camera shutter on every tracer (CameraData.has_close: each tracer's UpdateState(CameraData) sets camera, lens, then
        shutter): camera rays spread in time between the camera as it is and this close eye and frustum; under set_lens the close lens
        follows frustum_close and is focused at focus_close (default: the open focus).  The next set_camera drops it; set_lens keeps it.
        set_shutter(None) turns it off."""
        if eye_close is None:
            rc = self._lib.polaris_host_renderer_set_shutter(self._h, None, None, 0.0)
        else:
            e = np.ascontiguousarray(eye_close, dtype=np.float32).reshape(3)
            f = np.ascontiguousarray(frustum_close, dtype=np.float32).reshape(16)
            rc = self._lib.polaris_host_renderer_set_shutter(self._h, e.ctypes.data, f.ctypes.data, 0.0 if focus_close is None else float(focus_close))
        if rc:
            raise RuntimeError(f"set_shutter failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def set_projection(self, kind, height: float | None = None, lon_range: float = 2.0 * np.pi, lat_range: float = np.pi) -> None:
        """The camera projection on every tracer (CameraData.projection: each tracer's UpdateState(CameraData) sets camera, then
        projection, with the view basis of the frustum): "orthographic" with a window `height` world units high, or "equirect" spanning
        lon_range x lat_range radians, also by their T.PROJECTION_* numbers.  Every later set_camera keeps it.  set_projection(None)
        turns it off.  Refused while the lens or the shutter is on."""
        number = T.PROJECTION_PERSPECTIVE if kind is None else (T.PROJECTION_KINDS[kind] if isinstance(kind, str) else int(kind))
        if number == T.PROJECTION_ORTHOGRAPHIC and height is None:
            raise ValueError("an orthographic projection needs the height of its window")
        if self._lib.polaris_host_renderer_set_projection(self._h, number, float(height or 0.0), float(lon_range), float(lat_range)):
            raise RuntimeError(f"set_projection failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def read_aov(self, which: int) -> np.ndarray:
        """The primary's (H, W, 4) denoiser plane (polaris_hip_read_aov)."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        if self._lib.polaris_host_renderer_read_aov(self._h, int(which), out.ctypes.data, out.size):
            raise RuntimeError(f"read_aov failed: {self._lib.polaris_host_renderer_error(self._h).decode()}")
        return out

    def render(self, accumulated=0):
        rows = np.zeros(self.n, dtype=np.uint32)
        ms = C.c_double()
        rc = self._lib.polaris_host_renderer_render(self._h, accumulated, rows.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError(f"render failed ({rc}): {self._lib.polaris_host_renderer_error(self._h).decode()}")
        return [int(v) for v in rows], ms.value

    def tracer_stats(self, tracer_index: int):
        """(TraceStats, wall milliseconds) of tracer `tracer_index`'s last Trace."""
        st, ms = T.TraceStats(), C.c_double()
        if self._lib.polaris_host_renderer_tracer_stats(self._h, tracer_index, C.byref(st), C.byref(ms)):
            raise RuntimeError("tracer_stats: bad tracer index")
        return st, ms.value

    def merge_counts(self) -> dict:
        """Which branch the merges onto the primary took so far (polaris_hip_merge_counts)."""
        a = (C.c_uint64 * len(T.MERGE_BRANCHES))()
        if self._lib.polaris_host_renderer_merge_counts(self._h, a):
            raise RuntimeError("merge_counts failed")
        return {name: int(a[k]) for k, name in enumerate(T.MERGE_BRANCHES)}

    def read(self):
        fb = np.zeros((self.H, self.W, 4), dtype=np.uint8)
        acc = np.zeros((self.H, self.W, 4), dtype=np.float32)
        rc = self._lib.polaris_host_renderer_read(self._h, fb.ctypes.data, fb.size, acc.ctypes.data, acc.size)
        if rc:
            raise RuntimeError(f"read failed ({rc})")
        return fb, acc

    def save(self, path: str):
        """The SaveFrameBuffer post-process stage: the primary's RGBA8 frame buffer as a PNG."""
        rc = self._lib.polaris_host_renderer_save(self._h, path.encode())
        if rc:
            raise RuntimeError(f"save failed ({rc}): {self._lib.polaris_host_renderer_error(self._h).decode()}")

    def close(self):
        if self._h:
            self._lib.polaris_host_renderer_free(self._h)
            self._h = None

    __del__ = close


def denoise(frame_acc, weight: float, guide, albedo, *, block_y: int = 0, block_h: int | None = None, out=None,
            iterations: int = 4, normal_power_log2: int = 5, sigma_depth: float = 0.1, sigma_luminance: float = 4.0) -> np.ndarray:
    """polaris_host_denoise: the CPU restatement of the denoiser's filter (polaris_amd/host/denoise.cpp).  frame_acc, guide and
    albedo are (H, W, 4) float32; returns the DENOISED plane -- `out` (a copy of it) with the rows [block_y, block_y + block_h)
    written.  Raises ValueError where the library refuses the arguments."""
    lib = load()
    acc = np.ascontiguousarray(frame_acc, dtype=np.float32)
    g = np.ascontiguousarray(guide, dtype=np.float32)
    a = np.ascontiguousarray(albedo, dtype=np.float32)
    H, W = acc.shape[:2]
    if g.shape != acc.shape or a.shape != acc.shape or acc.shape != (H, W, 4):
        raise ValueError("denoise: frame_acc, guide and albedo must be (H, W, 4) of one size")
    res = np.zeros_like(acc) if out is None else np.array(out, dtype=np.float32, copy=True)
    if res.shape != acc.shape:
        raise ValueError("denoise: out must be (H, W, 4) like frame_acc")
    bh = H - block_y if block_h is None else block_h
    p = T.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_luminance)
    rc = lib.polaris_host_denoise(acc.ctypes.data, float(weight), g.ctypes.data, a.ctypes.data, W, H, int(block_y), int(bh), C.byref(p),
                                  res.ctypes.data)
    if rc:
        raise ValueError(f"denoise: bad arguments (code {rc})")
    return res


def _planes(name, *planes):
    out = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
    H, W = out[0].shape[:2]
    if any(a.shape != (H, W, 4) for a in out):
        raise ValueError(f"{name}: the planes must be (H, W, 4) float32 of one size")
    return out, H, W


def _own(name, a, H, W, dtype):
    """A caller's (H, W, 4) output plane as a copy the library may write (None: zeros)."""
    out = np.zeros((H, W, 4), dtype) if a is None else np.array(a, dtype=dtype, order="C", copy=True)
    if out.shape != (H, W, 4):
        raise ValueError(f"{name}: an output plane must be (H, W, 4) like the input")
    return out


def _reproject(name, call, history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, params, *, history_variance=None,
               moments=False, instances=None, tables=None, deform=None):
    """THE marshalling of every reprojection entry, host and device (tracer.py): the arguments as contiguous arrays of the right type
    and shape, then call(*C arguments) in the entry's order.  moments: polaris_host_reproject_moments' order (history_variance second);
    instances = (prev, current) INSTANCE planes with tables = (prev, current) inv_transform: the motion entries' order; deform = (hit,
    vertices, prev_vertices) behind it.  Null vertices and empty tables are passed on: the library refuses them.  Returns the PRIOR
    plane, or (PRIOR, PRIOR2) with history_variance.  ValueError on shapes no entry takes; `call` raises the entry's own error."""
    (hist, pg, pa, g, a), H, W = _planes(name, history, prev_guide, prev_albedo, guide, albedo)
    f = lambda x, *shape: np.ascontiguousarray(x, dtype=np.float32).reshape(*shape)  # noqa: E731
    pe, pf, e, fr = f(prev_eye, 3), f(prev_frustum, 16), f(eye, 3), f(frustum, 16)
    hv = None
    if history_variance is not None:
        (hv,), _, _ = _planes(name, history_variance)
        if hv.shape != hist.shape:
            raise ValueError(f"{name}: history_variance must be (H, W, 4) like the history")
    prior = np.zeros((H, W, 4), np.float32)
    prior2 = None if hv is None else np.zeros((H, W, 4), np.float32)
    p = T.temporal_params(*params)
    if instances is None:
        args = [hist, hv, pg, pa, pe, pf, g, a, e, fr, W, H, p, prior, prior2] if moments else [hist, pg, pa, pe, pf, g, a, e, fr, W, H, p, prior]
    else:
        pi, ci = (np.ascontiguousarray(x, np.uint32) for x in instances)
        pt, ct = (f(x, -1, 16) for x in tables)
        if pi.shape != (H, W) or ci.shape != (H, W) or pt.shape != ct.shape:
            raise ValueError(f"{name}: the INSTANCE planes must be (H, W), the two tables (n, 16)")
        args = [hist, pg, pa, pi, pe, pf, g, a, ci, e, fr, W, H, len(ct), pt, ct, p, hv, prior, prior2]
    if deform is not None:
        ht = np.ascontiguousarray(deform[0], np.uint32)
        v, pv = (None if x is None else f(x, -1, 4) for x in deform[1:])
        if ht.shape != (H, W, 4):
            raise ValueError(f"{name}: the HIT plane must be (H, W, 4)")
        if (v is not None and pv is not None and v.shape != pv.shape) or any(x is not None and len(x) % 3 for x in (v, pv)):
            raise ValueError(f"{name}: the two vertex arrays must be (3 NT, 4)")
        args += [ht, v, pv, 0 if v is None and pv is None else len(v if v is not None else pv) // 3]
    call(*[C.byref(x) if x is p else x.ctypes.data if isinstance(x, np.ndarray) else x for x in args])
    return prior if prior2 is None else (prior, prior2)


def _host_call(name):
    def call(*args):
        rc = getattr(load(), "polaris_host_" + name)(*args)
        if rc:
            raise ValueError(f"{name}: bad arguments (code {rc})")
    return call


def reproject(history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, *, max_history: int = 32,
              normal_threshold: float = 0.9, depth_threshold: float = 0.1) -> np.ndarray:
    """polaris_host_reproject: the CPU restatement of the temporal reprojection (polaris_amd/host/temporal.cpp).  The planes are
    (H, W, 4) float32, the cameras eye (3,) and frustum (4, 4) / (16,); returns the PRIOR plane (h rgb | m).  Raises ValueError where the library refuses the arguments."""
    return _reproject("reproject", _host_call("reproject"), history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, (max_history, normal_threshold, depth_threshold))


def reproject_moments(history, hvar, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, *, max_history: int = 32,
                      normal_threshold: float = 0.9, depth_threshold: float = 0.1) -> tuple[np.ndarray, np.ndarray]:
    """polaris_host_reproject_moments: reproject() plus the history VARIANCE plane's M2 -- returns (PRIOR, PRIOR2 = h2 | 0 | 0 | m)."""
    return _reproject("reproject_moments", _host_call("reproject_moments"), history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum,
                      (max_history, normal_threshold, depth_threshold), history_variance=hvar, moments=True)


def reproject_motion(history, prev_guide, prev_albedo, prev_instance, prev_eye, prev_frustum, guide, albedo, instance, eye, frustum,
                     prev_inv_transforms, inv_transforms, *, history_variance=None, max_history: int = 32, normal_threshold: float = 0.9,
                     depth_threshold: float = 0.1):
    """polaris_host_reproject_motion: reproject() with object motion -- the two (H, W) uint32 INSTANCE planes and the two (n, 16)
    inv_transform tables the history and the current frame were seen with.  Returns the PRIOR plane, or (PRIOR, PRIOR2) when the
    history's VARIANCE plane is given.  Raises ValueError where the library refuses the arguments."""
    return _reproject("reproject_motion", _host_call("reproject_motion"), history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum,
                      (max_history, normal_threshold, depth_threshold), history_variance=history_variance, instances=(prev_instance, instance), tables=(prev_inv_transforms, inv_transforms))


def reproject_deform(history, prev_guide, prev_albedo, prev_instance, prev_eye, prev_frustum, guide, albedo, instance, eye, frustum,
                     prev_inv_transforms, inv_transforms, hit, vertices, prev_vertices, *, history_variance=None, max_history: int = 32,
                     normal_threshold: float = 0.9, depth_threshold: float = 0.1):
    """polaris_host_reproject_deform: reproject_motion() with vertex motion -- the current (H, W, 4) uint32 HIT plane (scene triangle |
    bits of u | bits of v | 0) and the (3 NT, 4) vertices of the scene now and as the history saw them.  Returns the PRIOR plane, or
    (PRIOR, PRIOR2) when the history's VARIANCE plane is given.  Raises ValueError where the library refuses the arguments."""
    return _reproject("reproject_deform", _host_call("reproject_deform"), history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum,
                      (max_history, normal_threshold, depth_threshold), history_variance=history_variance, instances=(prev_instance, instance), tables=(prev_inv_transforms, inv_transforms),
                      deform=(hit, vertices, prev_vertices))


def reproject_projection(history, prev_guide, prev_albedo, prev_eye, guide, albedo, eye, projection, *, max_history: int = 32,
                         normal_threshold: float = 0.9, depth_threshold: float = 0.1) -> np.ndarray:
    """polaris_host_reproject_projection: reproject() under polaris_hip_set_projection -- the history camera and the current one share
    `projection` (a ctypes_api.ProjectionParams with kind != 0) and differ in the eye.  Returns the PRIOR plane."""
    planes = [np.ascontiguousarray(x, dtype=np.float32) for x in (history, prev_guide, prev_albedo, guide, albedo)]
    H, W = planes[0].shape[:2]
    if any(x.shape != (H, W, 4) for x in planes):
        raise ValueError("reproject_projection: the planes must all be (H, W, 4)")
    e0, e1 = (np.ascontiguousarray(x, dtype=np.float32).reshape(3) for x in (prev_eye, eye))
    prior = np.zeros((H, W, 4), np.float32)
    p = T.temporal_params(max_history, normal_threshold, depth_threshold)
    _host_call("reproject_projection")(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, e0.ctypes.data, planes[3].ctypes.data,
                                       planes[4].ctypes.data, e1.ctypes.data, C.byref(projection), W, H, C.byref(p), prior.ctypes.data)
    return prior


def projection_rays(projection, eye, W: int, H: int) -> tuple[np.ndarray, np.ndarray]:
    """polaris_host_projection_rays: (origins, directions), each (H * W, 3) float32 -- the guide ray through every pixel's centre under
    `projection`, from the header the G-buffer kernels use (polaris_amd/csrc/temporal.h, tp_guide_ray)."""
    e = np.ascontiguousarray(eye, dtype=np.float32).reshape(3)
    o, d = np.zeros((H * W, 3), np.float32), np.zeros((H * W, 3), np.float32)
    _host_call("projection_rays")(C.byref(projection), e.ctypes.data, W, H, o.ctypes.data, d.ctypes.data)
    return o, d


def projection_project(projection, eye, points) -> tuple[np.ndarray, np.ndarray]:
    """polaris_host_projection_project: tp_project of the projected camera for (n, 3) points -- ((n, 3) u | v | dist, (n,) bool ok)."""
    e = np.ascontiguousarray(eye, dtype=np.float32).reshape(3)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    uvd, ok = np.zeros((pts.shape[0], 3), np.float32), np.zeros(pts.shape[0], np.uint8)
    _host_call("projection_project")(C.byref(projection), e.ctypes.data, pts.ctypes.data, pts.shape[0], uvd.ctypes.data, ok.ctypes.data)
    return uvd, ok.astype(bool)


MOTION_STATIC, MOTION_MOVED, MOTION_INVALID = 0, 1, 2


def motion_matrix(inv_hist, inv_cur) -> tuple[int, np.ndarray]:
    """tp_motion_matrix (polaris_amd/csrc/temporal.h), the function the library builds its motion table with: (flag, D (3, 4) float32)
    of one mesh instance from its two inv_transform (16 floats, column major): MOTION_STATIC when they are byte-equal, MOTION_MOVED
    with D = inverse(Inv_hist) . Inv_cur, or MOTION_INVALID."""
    a = np.ascontiguousarray(inv_hist, dtype=np.float32).reshape(16)
    b = np.ascontiguousarray(inv_cur, dtype=np.float32).reshape(16)
    flag, D = C.c_uint32(), np.zeros((3, 4), np.float32)
    if load().polaris_host_motion_matrix(a.ctypes.data, b.ctypes.data, C.byref(flag), D.ctypes.data):
        raise ValueError("motion_matrix: bad arguments")
    return int(flag.value), D


def temporal_combine(frame_acc, prior, accumulated_samples: int, samples_per_pixel: int, *, block_y: int = 0, block_h: int | None = None,
                     out=None) -> np.ndarray:
    """polaris_host_temporal_combine: the TEMPORAL plane (rgb | n + m) of the rows [block_y, block_y + block_h) of a sync with these
    sample counts; the other rows as `out` gave them (zeros by default)."""
    acc = np.ascontiguousarray(frame_acc, dtype=np.float32)
    pr = np.ascontiguousarray(prior, dtype=np.float32)
    H, W = acc.shape[:2]
    if pr.shape != acc.shape or acc.shape != (H, W, 4):
        raise ValueError("temporal_combine: frame_acc and prior must be (H, W, 4) of one size")
    res = np.zeros_like(acc) if out is None else np.array(out, dtype=np.float32, copy=True)
    bh = H - block_y if block_h is None else block_h
    rc = load().polaris_host_temporal_combine(acc.ctypes.data, pr.ctypes.data, int(accumulated_samples), int(samples_per_pixel), W, H,
                                              int(block_y), int(bh), res.ctypes.data)
    if rc:
        raise ValueError(f"temporal_combine: bad arguments (code {rc})")
    return res


def exposure_info(info) -> dict:
    """A PolarisExposureInfo as a dict: valid, n_metered and the float32 values avg, log2E, E."""
    return {"valid": int(info.valid), "n_metered": int(info.n_metered), "avg": np.float32(info.avg), "log2E": np.float32(info.log2E), "E": np.float32(info.E)}


def display(plane, *, weight: float = 1.0, exposure: float = 1.0, block_y: int = 0, block_h: int | None = None, rgba=None, prev_log2E=None,
            **fields) -> tuple[np.ndarray, np.ndarray, dict]:
    """polaris_host_display: the CPU restatement of the display stage (polaris_amd/host/display.cpp) over the request's rows of an
    (H, W, 4) float32 plane.  fields: those of ctypes_api.DISPLAY_DEFAULTS.  Returns (RGBA8 -- `rgba` (a copy) with the request's rows
    written --, the 256 counts, exposure_info).  ValueError where refused."""
    (c,), H, W = _planes("display", plane)
    fb = _own("display", rgba, H, W, np.uint8)
    p, info, hist = T.display_params(1, **fields), T.ExposureInfo(), np.zeros(256, np.uint32)
    prev = None if prev_log2E is None else C.byref(C.c_float(float(prev_log2E)))
    rc = load().polaris_host_display(c.ctypes.data, W, H, int(block_y), int(H - block_y if block_h is None else block_h), float(weight), float(exposure),
                                     C.byref(p), prev, fb.ctypes.data, hist.ctypes.data, C.byref(info))
    if rc:
        raise ValueError(f"display: bad arguments (code {rc})")
    return fb, hist, exposure_info(info)


def bloom_levels(W: int, rows: int, levels: int) -> tuple[int, int, int]:
    """(levels used, w_1, h_1) of the bloom pyramid over a region W x rows with `levels` asked for (bloom.h bl_levels)."""
    w1, h1 = C.c_uint32(), C.c_uint32()
    L = load().polaris_host_bloom_levels(int(W), int(rows), int(levels), C.byref(w1), C.byref(h1))
    return int(L), int(w1.value), int(h1.value)


def bloom(plane, *, weight: float = 1.0, exposure: float = 1.0, block_y: int = 0, block_h: int | None = None, rgba=None, prev_log2E=None,
          display: dict | None = None, **fields) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """polaris_host_bloom: the CPU restatement of a bloomed displayed sync (polaris_amd/host/bloom.cpp) over the request's rows of an
    (H, W, 4) float32 plane.  display: fields of ctypes_api.DISPLAY_DEFAULTS; fields: those of ctypes_api.BLOOM_DEFAULTS.  Returns
    (RGBA8 -- `rgba` (a copy) with the request's rows written --, U_1 (h_1, w_1, 4), the full-resolution term of the request's rows
    (block_h, W, 4), levels used).  ValueError where refused."""
    (c,), H, W = _planes("bloom", plane)
    fb = _own("bloom", rgba, H, W, np.uint8)
    bh = int(H - block_y if block_h is None else block_h)
    dp, bp = T.display_params(1, **(display or {})), T.bloom_params(1, **fields)
    if not (0 <= block_y < H and 0 < bh <= H - block_y) or load().polaris_host_bloom_check(C.byref(bp)):
        raise ValueError("bloom: bad rows or bloom params")
    L, w1, h1 = bloom_levels(W, bh, bp.levels)
    u1, term, used = np.zeros((h1, w1, 4), np.float32), np.zeros((bh, W, 4), np.float32), C.c_uint32()
    prev = None if prev_log2E is None else C.byref(C.c_float(float(prev_log2E)))
    rc = load().polaris_host_bloom(c.ctypes.data, W, H, int(block_y), bh, float(weight), float(exposure), C.byref(dp), C.byref(bp), prev, fb.ctypes.data,
                                   u1.ctypes.data, term.ctypes.data, C.byref(used))
    if rc:
        raise ValueError(f"bloom: bad arguments (code {rc})")
    assert used.value == L
    return fb, u1, term, L


def variance(frame_acc, samples: int, guide, albedo, *, temporal=None, prior2=None, block_y: int = 0, block_h: int | None = None, out=None,
             normal_power_log2: int = 5, sigma_depth: float = 0.1, sigma_variance: float = 8.0, min_samples: int = 8) -> np.ndarray:
    """polaris_host_variance: the CPU restatement of k_variance (polaris_amd/host/variance.cpp).  frame_acc (rgb | sum L^2 of `samples`
    samples), guide and albedo are (H, W, 4) float32; with temporal reuse the TEMPORAL plane and PRIOR2 are given too.  Returns the
    VARIANCE plane (M1 | M2 | n_eff | v) -- `out` (a copy of it) with the request's rows written.  ValueError where refused."""
    (acc, g, a), H, W = _planes("variance", frame_acc, guide, albedo)
    tp = p2 = None
    if temporal is not None or prior2 is not None:
        (tp, p2), _, _ = _planes("variance", temporal, prior2)
        if tp.shape != acc.shape:
            raise ValueError("variance: temporal / prior2 must be (H, W, 4) like frame_acc")
    res = np.zeros_like(acc) if out is None else np.array(out, dtype=np.float32, copy=True)
    bh = H - block_y if block_h is None else block_h
    p = T.denoise_params(1, normal_power_log2, sigma_depth, 0.0)
    v = T.variance_params(sigma_variance, min_samples)
    rc = load().polaris_host_variance(acc.ctypes.data, int(samples), None if tp is None else tp.ctypes.data, None if p2 is None else p2.ctypes.data,
                                      g.ctypes.data, a.ctypes.data, W, H, int(block_y), int(bh), C.byref(p), C.byref(v), res.ctypes.data)
    if rc:
        raise ValueError(f"variance: bad arguments (code {rc})")
    return res


def denoise_variance(acc, weight: float, variance_plane, guide, albedo, *, block_y: int = 0, block_h: int | None = None, out=None,
                     iterations: int = 4, normal_power_log2: int = 5, sigma_depth: float = 0.1, sigma_variance: float = 8.0,
                     min_samples: int = 8) -> np.ndarray:
    """polaris_host_denoise_variance: the CPU restatement of the variance-guided filter (polaris_amd/host/variance.cpp) over acc *
    weight with the VARIANCE plane.  Returns the DENOISED plane (rgb | filtered variance) -- `out` (a copy) with the request's rows
    written.  ValueError where refused."""
    (c, vp, g, a), H, W = _planes("denoise_variance", acc, variance_plane, guide, albedo)
    res = np.zeros_like(c) if out is None else np.array(out, dtype=np.float32, copy=True)
    bh = H - block_y if block_h is None else block_h
    p = T.denoise_params(iterations, normal_power_log2, sigma_depth, 0.0)
    v = T.variance_params(sigma_variance, min_samples)
    rc = load().polaris_host_denoise_variance(c.ctypes.data, float(weight), vp.ctypes.data, g.ctypes.data, a.ctypes.data, W, H, int(block_y),
                                              int(bh), C.byref(p), C.byref(v), res.ctypes.data)
    if rc:
        raise ValueError(f"denoise_variance: bad arguments (code {rc})")
    return res


CAMERA_MOVES = {"up": 0, "down": 1, "left": 2, "right": 3, "forward": 4, "backward": 5}   # scene.CameraDirection (camera.go:12-19)


def camera_move(camera: dict, moves, *, aspect: float = 1.0, invert_y: bool = False):
    """polaris_host_camera_move: (eye (3,), frustum (4, 4)) of the camera `camera` (read_scene's .camera dict) after the moves
    [(direction name, offset), ...] of scene.Camera.Move on one camera object, as the interactive renderer makes them."""
    params = np.concatenate([[camera["fov"]], camera["eye"], camera["look"], camera["up"]]).astype(np.float32)
    dirs = np.ascontiguousarray([CAMERA_MOVES[d] for d, _ in moves], dtype=np.int32)
    offs = np.ascontiguousarray([o for _, o in moves], dtype=np.float32)
    eye = np.zeros(3, np.float32)
    fr = np.zeros((4, 4), np.float32)
    if load().polaris_host_camera_move(params.ctypes.data, float(aspect), int(invert_y), dirs.ctypes.data, offs.ctypes.data, len(dirs), None,
                                       eye.ctypes.data, fr.ctypes.data):
        raise ValueError("camera_move: bad arguments")
    return eye, fr


def bvh_build(boxes, min_leaf: int):
    """bvh.Build (asset/compiler/bvh/bvh_builder.go:100-124) over boxes (n, 6) = min.xyz, max.xyz.
    Returns (nodes as T.BVH_NODE array, list of leaf sizes in callback order)."""
    lib = load()
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    cap = 2 * len(b) + 1
    nodes = np.zeros(cap, dtype=T.BVH_NODE)
    sizes = np.zeros(cap, dtype=np.uint32)
    nl = C.c_uint32()
    n = lib.polaris_host_bvh_build(b.ctypes.data, len(b), min_leaf, nodes.ctypes.data, cap, sizes.ctypes.data, C.byref(nl))
    return nodes[:n].copy(), [int(v) for v in sizes[: nl.value]]


def _scene_from_handle(lib, h, name):
    """Copy the arrays of a compiled scene (CompiledBox handle) into a polaris_amd.scenes.Scene."""
    from .scenes import Scene

    v = lib.polaris_host_compiled_view(h).contents

    def grab(ptr, count, dtype):
        if not ptr or count == 0:
            return np.zeros(0, dtype=dtype)
        nbytes = count * np.dtype(dtype).itemsize
        return np.frombuffer(C.string_at(ptr, nbytes), dtype=dtype).copy()

    nt = v.num_triangles
    return Scene(
        bvh_nodes=grab(v.bvh_nodes, v.num_bvh_nodes, T.BVH_NODE), mesh_instances=grab(v.mesh_instances, v.num_mesh_instances, T.MESH_INSTANCE),
        material_nodes=grab(v.material_nodes, v.num_material_nodes, T.MATERIAL_NODE), emissives=grab(v.emissives, v.num_emissives, T.EMISSIVE),
        texture_data=grab(v.texture_data, v.texture_data_bytes, np.uint8), texture_meta=grab(v.texture_meta, v.num_textures, T.TEXTURE_META),
        vertices=grab(v.vertices, nt * 12, np.float32).reshape(-1, 4), normals=grab(v.normals, nt * 12, np.float32).reshape(-1, 4),
        uvs=grab(v.uvs, nt * 6, np.float32).reshape(-1, 2), material_index=grab(v.material_index, nt, np.uint32),
        scene_diffuse_mat_index=int(v.scene_diffuse_mat_index), scene_emissive_mat_index=int(v.scene_emissive_mat_index), name=name)


def compile_scene(meshes, instances, mats, *, scene_diffuse=-1, scene_emissive=-1, min_leaf=10, name="compiled"):
    """The C++ scene compiler (polaris_amd/host/scene_compiler.cpp = compiler.go partitionGeometry) on
    the same inputs polaris_amd.scenes.compile_scene takes: list[scenes.Mesh], list[(mesh index, 4x4
    world matrix)], scenes.MaterialTable (per-triangle `mat` values are material root nodes).
    Returns a polaris_amd.scenes.Scene holding copies of the compiled arrays."""
    from .scenes import Scene

    lib = load()
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    V = f32(np.concatenate([m.verts for m in meshes]))
    Nn = f32(np.concatenate([m.normals for m in meshes]))
    U = f32(np.concatenate([m.uvs for m in meshes]))
    roots = sorted({int(r) for m in meshes for r in np.asarray(m.mat)})
    root_to_mat = {r: i for i, r in enumerate(roots)}
    M = np.ascontiguousarray([root_to_mat[int(r)] for m in meshes for r in np.asarray(m.mat)], dtype=np.int32)
    offs = np.zeros(len(meshes) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(m.verts) for m in meshes])
    inst_mesh = np.ascontiguousarray([i for i, _ in instances], dtype=np.uint32)
    inst_xf = f32(np.stack([np.asarray(x, dtype=np.float64).T.reshape(-1) for _, x in instances]))  # column major
    nodes, tex_meta, tex_blob = mats.arrays()
    mroots = np.ascontiguousarray(roots, dtype=np.int32)
    err = C.create_string_buffer(256)
    h = lib.polaris_host_compile_scene(V.ctypes.data, Nn.ctypes.data, U.ctypes.data, M.ctypes.data, offs.ctypes.data, len(meshes),
                                       inst_mesh.ctypes.data, inst_xf.ctypes.data, len(instances), nodes.ctypes.data, len(nodes),
                                       mroots.ctypes.data, len(mroots), T._ptr(tex_meta), len(tex_meta), T._ptr(tex_blob), tex_blob.size,
                                       scene_diffuse, scene_emissive, min_leaf, err)
    if not h:
        raise RuntimeError(f"compile_scene: {err.value.decode()}")
    try:
        sc = _scene_from_handle(lib, h, name)
    finally:
        lib.polaris_host_compiled_free(h)
    return sc


# ---- scene front-end: Wavefront OBJ/MTL reader, material expressions, textures ------------------
def material_check(expr: str):
    """(status, message): 0 valid, 1 parse error, 2 semantic error (material.ParseExpression + Validate)."""
    err = C.create_string_buffer(512)
    rc = load().polaris_host_material_check(expr.encode(), err)
    return rc, err.value.decode()


def material_ior(name: str):
    out = C.c_float()
    return None if load().polaris_host_material_ior(name.encode(), C.byref(out)) else float(out.value)


def read_scene(path=None, *, content=None, name="embedded", aspect=1.0, invert_y=False, min_leaf=0):
    """reader.ReadScene: parse a Wavefront .obj (+ .mtl, textures) and compile it.  Returns a
    polaris_amd.scenes.Scene whose eye/frustum come from the file's camera_* statements for a frame of
    the given aspect; `.camera` = dict(fov, eye, look, up), `.warnings` = list of strings."""
    lib = load()
    err = C.create_string_buffer(1024)
    h = lib.polaris_host_read_scene(path.encode() if path is not None else None, name.encode(),
                                    content.encode() if content is not None else None, min_leaf, err)
    if not h:
        raise RuntimeError(err.value.decode())
    try:
        sc = _scene_from_handle(lib, h, os.path.basename(path) if path else name)
        params = np.zeros(10, np.float32)
        eye = np.zeros(3, np.float32)
        fr = np.zeros((4, 4), np.float32)
        lib.polaris_host_compiled_camera(h, float(aspect), int(invert_y), params.ctypes.data, eye.ctypes.data, fr.ctypes.data)
        sc.eye, sc.frustum = eye, fr
        sc.camera = {"fov": float(params[0]), "eye": params[1:4].copy(), "look": params[4:7].copy(), "up": params[7:10].copy()}
        n = lib.polaris_host_compiled_warnings(h, None, 0)
        buf = C.create_string_buffer(n + 1)
        lib.polaris_host_compiled_warnings(h, buf, n + 1)
        sc.warnings = [w for w in buf.value.decode().split("\n") if w]
    finally:
        lib.polaris_host_compiled_free(h)
    return sc


def parse_obj(content: str, max_instances=64):
    """Parse-level view of an .obj: dict(counts, transforms [n][4][4] (row = matrix row), boxes, materials)."""
    counts = np.zeros(4, np.uint32)
    xf = np.zeros((max_instances, 16), np.float32)
    boxes = np.zeros((max_instances, 9), np.float32)
    mats = C.create_string_buffer(1 << 16)
    err = C.create_string_buffer(1024)
    if load().polaris_host_parse_obj(content.encode(), counts.ctypes.data, xf.ctypes.data, boxes.ctypes.data, max_instances, mats, len(mats), err):
        raise RuntimeError(err.value.decode())
    n = int(counts[1])
    materials = [tuple(l.split("\t")) for l in mats.value.decode().split("\n") if l]
    return {"meshes": int(counts[0]), "instances": n, "materials": materials, "mesh0_primitives": int(counts[3]),
            "transforms": xf[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), "bbox": boxes[:n, :6].reshape(n, 2, 3).copy(), "center": boxes[:n, 6:].copy()}


def parse_mtl(content: str):
    """[(name, generated material expression)] of a material library (parseMaterials + GetExpression)."""
    mats = C.create_string_buffer(1 << 16)
    err = C.create_string_buffer(1024)
    if load().polaris_host_parse_mtl(content.encode(), mats, len(mats), err):
        raise RuntimeError(err.value.decode())
    return [tuple(l.split("\t")) for l in mats.value.decode().split("\n") if l]


def select_face_index(token: str, list_len: int, rel_offset: int = 0):
    out = C.c_int(-1)
    err = C.create_string_buffer(256)
    if load().polaris_host_select_face_index(token.encode(), list_len, rel_offset, C.byref(out), err):
        raise ValueError(err.value.decode())
    return out.value


def texture_load(path: str):
    """(format, width, height, texel bytes) of an image file as the scene compiler bakes it."""
    meta = np.zeros(4, np.uint32)
    err = C.create_string_buffer(512)
    lib = load()
    if lib.polaris_host_texture_load(path.encode(), meta.ctypes.data, None, 0, err):
        raise RuntimeError(err.value.decode())
    data = np.zeros(int(meta[3]), np.uint8)
    lib.polaris_host_texture_load(path.encode(), meta.ctypes.data, data.ctypes.data, data.size, err)
    return int(meta[0]), int(meta[1]), int(meta[2]), data


def write_png(path: str, rgba: np.ndarray):
    """renderer::WritePNG: (h, w, 4) uint8 -> PNG file (the encoder behind Renderer.save)."""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = a.shape[:2]
    if load().polaris_host_write_png(path.encode(), a.ctypes.data, w, h):
        raise RuntimeError(f"write_png: could not write {path}")
