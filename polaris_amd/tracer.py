"""Host-side mirror of the reference's tracer.Tracer interface over the C ABI (ctypes).

Same method names, argument meaning and error behaviour as tracer/tracer.go:80-111 and its
OpenCL implementation tracer/opencl/tracer.go, so tests and bench.py drive the HIP backend the way
renderer/default.go drives a tracer.  This module is plumbing only: every method is one call into
libpolaris_hip.so (include/polaris_hip.h); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import enum
import time
from dataclasses import dataclass

import numpy as np

from . import ctypes_api as T
from . import host_api as HA   # (the marshalling the device entries share with their CPU restatements; no library is loaded by the import)


class Flag(enum.IntFlag):          # tracer/tracer.go:49-61
    Local = 1
    Remote = 2
    CpuDevice = 4


class UpdateMode(enum.IntEnum):    # tracer/tracer.go:63-69
    Synchronous = 0
    Asynchronous = 1


class ChangeType(enum.IntEnum):    # tracer/tracer.go:71-78
    FrameDimensions = 0
    SceneData = 1
    CameraData = 2


@dataclass
class Stats:                       # tracer/tracer.go:37-47 (durations in seconds)
    BlockW: int = 0
    BlockH: int = 0
    UpdateTime: float = 0.0
    RenderTime: float = 0.0


class TracerError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"polaris_hip error {code}: {msg}")
        self.code = code


class ErrNoSceneData(TracerError):  # tracer/opencl/errors.go
    pass


E_NO_SCENE_DATA = 1


class HipTracer:
    """tracer.Tracer implemented on one MI355X through the C ABI."""

    def __init__(self, id: str, device_index: int = 0, lib_path: str | None = None):
        self._lib = T.load_library(lib_path)
        self._id = id
        self._device = device_index
        self._h = C.c_void_p()
        self._stats = Stats()
        self._changes: dict[ChangeType, object] = {}
        self._name = ""
        self._speed = 0
        self.last_trace_stats: T.TraceStats | None = None
        self._keepalive = None
        self._camera = None   # the CameraData last committed (set_lens derives its vectors from it)
        self._lens = None     # (radius, focus_distance) of set_lens: re-applied after every camera update
        self._shutter = None  # (eye_close, frustum_close, focus_close) of set_shutter: forgotten at every camera update, re-sent after a set_lens
        self._projection = None  # (kind, height, lon_range, lat_range) of set_projection: re-sent with the new basis after every camera update

    # ---- tracer.Tracer ---------------------------------------------------------------------
    def Id(self) -> str:
        return self._id

    def Flags(self) -> Flag:
        return Flag.Local

    def Speed(self) -> int:
        """compute units * MHz / 1000 (tracer/opencl/device/device.go:219)."""
        return self._speed

    def Init(self) -> None:
        T.check_load_order(self._lib)
        name = C.create_string_buffer(256)
        cus, mhz, mem = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self._lib.polaris_hip_device_info(self._device, name, C.byref(cus), C.byref(mhz), C.byref(mem)), None)
        self._name = name.value.decode()
        self._speed = int(cus.value * mhz.value // 1000)
        self.device_cus = int(cus.value)   # compute units of the device (bench.py: the issue roofline's peak)
        self._check(self._lib.polaris_hip_create(self._device, C.byref(self._h)), None)

    def Close(self) -> None:
        if self._h:
            self._lib.polaris_hip_destroy(self._h)
            self._h = C.c_void_p()

    def Stats(self) -> Stats:
        return self._stats

    def UpdateState(self, mode: UpdateMode, change: ChangeType, data) -> float:
        """Queue a state change; Synchronous commits at once, Asynchronous at the next Trace
        (tracer/opencl/tracer.go:150-192)."""
        self._changes[ChangeType(change)] = data
        if mode == UpdateMode.Synchronous:
            return self._commit()
        return 0.0

    def Trace(self, req: T.BlockRequest, seeds: np.ndarray | None = None) -> float:
        """tracer/opencl/tracer.go:194-247.  `seeds` stands in for the Go math/rand draws (one
        per sample + one per bounce); if omitted they are drawn from numpy's global RNG the way
        the reference draws from math/rand."""
        t0 = time.perf_counter()
        self._commit()
        n = req.samples_per_pixel * (1 + req.num_bounces)
        if seeds is None:
            seeds = np.random.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        st = T.TraceStats()
        rc = self._lib.polaris_hip_trace(self._h, C.byref(req), seeds.ctypes.data_as(C.POINTER(C.c_uint32)), seeds.size, C.byref(st))
        self._check(rc, self._h)
        self.last_trace_stats = st
        req.accumulated_samples += req.samples_per_pixel  # tracer.go:240 (on the caller's copy)
        self._stats.BlockW, self._stats.BlockH = req.block_w, req.block_h
        self._stats.RenderTime = time.perf_counter() - t0
        return self._stats.RenderTime

    def MergeOutput(self, other: "HipTracer", req: T.BlockRequest) -> float:
        t0 = time.perf_counter()
        if not isinstance(other, HipTracer):  # tracer.go:280-283
            raise TracerError(6, "merge failed: unsupported tracer instance")
        self._check(self._lib.polaris_hip_merge(self._h, other._h, C.byref(req)), self._h)
        return time.perf_counter() - t0

    def SyncFramebuffer(self, req: T.BlockRequest) -> float:
        t0 = time.perf_counter()
        self._check(self._lib.polaris_hip_sync_framebuffer(self._h, C.byref(req)), self._h)
        return time.perf_counter() - t0

    # ---- extras used by tests / bench --------------------------------------------------------
    def set_option(self, key: str, value: int) -> None:
        self._check(self._lib.polaris_hip_set_option(self._h, key.encode(), int(value)), self._h)

    def read_accumulator(self, which: int = 0) -> np.ndarray:
        out = np.zeros((self._H, self._W, 4), dtype=np.float32)
        self._check(self._lib.polaris_hip_read_accumulator(self._h, which, out.ctypes.data, out.size), self._h)
        return out

    def set_denoise(self, iterations: int = 4, normal_power_log2: int = 5, sigma_depth: float = 0.1, sigma_luminance: float = 4.0) -> None:
        """Denoise the frame at every SyncFramebuffer (polaris_hip_set_denoise); iterations = 0 turns it off (the default)."""
        p = T.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_luminance)
        self._check(self._lib.polaris_hip_set_denoise(self._h, C.byref(p)), self._h)

    def set_temporal(self, max_history: int = 32, normal_threshold: float = 0.9, depth_threshold: float = 0.1) -> None:
        """Reuse the last view's mean across camera moves at every SyncFramebuffer (polaris_hip_set_temporal); max_history = 0 turns
        it off (the default) and drops the history."""
        p = T.temporal_params(max_history, normal_threshold, depth_threshold)
        self._check(self._lib.polaris_hip_set_temporal(self._h, C.byref(p)), self._h)

    def set_lens(self, radius: float, focus_distance: float = 0.0) -> None:
        """Thin-lens camera (polaris_hip_set_lens): a round lens of this radius focused at this distance along the view axis, with
        the vectors of T.lens_from_frustum on the camera last given through UpdateState; re-applied after every later camera update.
        radius = 0 turns the lens off (the default).  The caller restarts accumulation, as after a camera change."""
        self._commit()
        self._lens = (float(radius), float(focus_distance)) if radius != 0 else None
        if self._lens is None:
            self.set_lens_vectors(0.0, (0, 0, 0), (0, 0, 0), (0, 0, 0))
        else:
            self._apply_lens()
        if self._shutter is not None:   # (a changed lens switched the shutter off: it comes back with the close lens of the new one)
            self._apply_shutter()

    def set_lens_vectors(self, focus_distance: float, axis, u, v) -> None:
        """The raw call: a lens point is eye + lx u + ly v, (lx, ly) uniform in the unit disk; u = v = 0 turns the lens off."""
        p = T.lens_params(focus_distance, axis, u, v)
        self._check(self._lib.polaris_hip_set_lens(self._h, C.byref(p)), self._h)

    def _apply_lens(self) -> None:
        if self._camera is None:
            raise TracerError(2, "set_lens: no camera given through UpdateState yet")
        axis, u, v = T.lens_from_frustum(self._camera.frustum, self._lens[0])
        self.set_lens_vectors(self._lens[1], axis, u, v)

    def set_shutter(self, eye_close, frustum_close=None, focus_close: float | None = None) -> None:
        """Camera shutter (polaris_hip_set_shutter): every camera ray gets its own time in [0, 1) between the camera last given through
        UpdateState (shutter open) and this eye and frustum (shutter close) -- camera motion blur.  With set_lens(radius, focus)
        active the close lens has the vectors of T.lens_from_frustum(frustum_close, radius) and is focused at focus_close (default: the
        open focus) -- a focus pull.  set_shutter(None) turns it off (the default).  The close camera belongs to the open one: a camera
        update through UpdateState forgets the shutter; a set_lens re-sends it with the new close lens.  The caller restarts accumulation.
        (A lens given through set_lens_vectors is not known here: its close lens goes through set_shutter_params.)"""
        self._commit()
        if eye_close is None:
            self._shutter = None
            self.set_shutter_params(T.shutter_params())
            return
        if frustum_close is None:
            raise TracerError(2, "set_shutter: a close eye needs a close frustum")
        self._shutter = (np.array(eye_close, np.float32).reshape(3), np.array(frustum_close, np.float32).reshape(16),
                         None if focus_close is None else float(focus_close))
        self._apply_shutter()

    def set_shutter_params(self, p: T.ShutterParams) -> None:
        """The raw call (T.shutter_params builds the struct)."""
        self._check(self._lib.polaris_hip_set_shutter(self._h, C.byref(p)), self._h)

    def _apply_shutter(self) -> None:
        eye1, frustum1, focus1 = self._shutter
        if self._lens is None:
            self.set_shutter_params(T.shutter_params(eye1, frustum1))
        else:
            axis1, u1, v1 = T.lens_from_frustum(frustum1, self._lens[0])
            self.set_shutter_params(T.shutter_params(eye1, frustum1, self._lens[1] if focus1 is None else focus1, axis1, u1, v1))

    def set_projection(self, kind, height: float | None = None, lon_range: float = 2.0 * np.pi, lat_range: float = np.pi) -> None:
        """Camera projection (polaris_hip_set_projection): kind "orthographic" (a window `height` world units high through the eye, as
        wide as the frustum's aspect makes it) or "equirect" (a lon_range x lat_range radians panorama), also by their T.PROJECTION_*
        numbers, looking along the view basis of the camera last given through UpdateState (T.projection_from_frustum); re-sent with the
        new basis after every later camera update.  set_projection(None) (or "perspective") turns it off (the default).  Refused with the
        lens or the shutter on.  The caller restarts accumulation, as after a camera change."""
        self._commit()
        number = T.PROJECTION_PERSPECTIVE if kind is None else (T.PROJECTION_KINDS[kind] if isinstance(kind, str) else int(kind))
        if number == T.PROJECTION_PERSPECTIVE:
            self._projection = None
            self.set_projection_params(T.projection_params())
            return
        previous, self._projection = self._projection, (number, height, float(lon_range), float(lat_range))
        try:
            self._apply_projection()
        except (TracerError, ValueError):
            self._projection = previous   # (a refusal changed nothing in the library)
            raise

    def set_projection_params(self, p: T.ProjectionParams) -> None:
        """The raw call (T.projection_params builds the struct): the basis is the caller's and is not re-derived at a camera update."""
        self._check(self._lib.polaris_hip_set_projection(self._h, C.byref(p)), self._h)

    def _apply_projection(self) -> None:
        if self._camera is None:
            raise TracerError(2, "set_projection: no camera given through UpdateState yet")
        kind, height, lon_range, lat_range = self._projection
        self.set_projection_params(T.projection_for(kind, self._camera.frustum, height, lon_range, lat_range))

    def set_variance(self, sigma_variance: float = 8.0, min_samples: int = 8) -> None:
        """Variance-guided denoising at every SyncFramebuffer (polaris_hip_set_variance): turns the option "moments" on first, then
        sets the params; sigma_variance = 0 turns guidance off (the default) and leaves "moments" as it is."""
        if sigma_variance != 0:
            self.set_option("moments", 1)
        p = T.variance_params(sigma_variance, min_samples)
        self._check(self._lib.polaris_hip_set_variance(self._h, C.byref(p)), self._h)

    def set_display(self, enabled: int = 1, **fields) -> None:
        """The display transform of every SyncFramebuffer (polaris_hip_set_display): auto-exposure, tone operator and transfer function
        in place of the plain tone-map.  fields: those of T.DISPLAY_DEFAULTS (tone_operator also by its T.TONE_OPERATORS name);
        enabled = 0 turns it off (the default)."""
        p = T.display_params(enabled, **fields)
        self._check(self._lib.polaris_hip_set_display(self._h, C.byref(p)), self._h)

    def set_bloom(self, enabled: int = 1, **fields) -> None:
        """The bloom of the display transform (polaris_hip_set_bloom): a bright-pass pyramid added before the tone curve, in effect while
        set_display is on.  fields: those of T.BLOOM_DEFAULTS; enabled = 0 turns it off (the default)."""
        p = T.bloom_params(enabled, **fields)
        self._check(self._lib.polaris_hip_set_bloom(self._h, C.byref(p)), self._h)

    def bloom_planes(self, plane, *, weight: float = 1.0, exposure: float = 1.0, block_y: int = 0, block_h: int | None = None, rgba=None,
                     prev_log2E=None, display: dict | None = None, **fields) -> tuple[np.ndarray, np.ndarray, int]:
        """polaris_hip_bloom_planes: the launches of a bloomed displayed sync on a caller (H, W, 4) float32 plane.  display: fields of
        T.DISPLAY_DEFAULTS; fields: those of T.BLOOM_DEFAULTS.  Returns (RGBA8, U_1 (h_1, w_1, 4), levels used); rows outside the
        request come back as passed (zeros by default)."""
        (plane,), H, W = HA._planes("bloom_planes", plane)
        fb = HA._own("bloom_planes", rgba, H, W, np.uint8)
        bh = int(H - block_y if block_h is None else block_h)
        dp, bp, used = T.display_params(1, **(display or {})), T.bloom_params(1, **fields), C.c_uint32()
        w1, h1 = (W + 1) // 2, (max(bh, 1) + 1) // 2
        u1 = np.zeros((h1, w1, 4), np.float32)
        prev = None if prev_log2E is None else C.byref(C.c_float(float(prev_log2E)))
        self._check(self._lib.polaris_hip_bloom_planes(self._h, plane.ctypes.data, W, H, int(block_y), bh, float(weight), float(exposure), C.byref(dp),
                                                       C.byref(bp), prev, fb.ctypes.data, u1.ctypes.data, C.byref(used)), self._h)
        return fb, u1, int(used.value)

    def read_exposure(self) -> dict:
        """polaris_hip_read_exposure: what the last sync with auto-exposure on metered -- valid, n_metered, the float32 values avg,
        log2E and E, and the 256 counts under "histogram"."""
        info, hist = T.ExposureInfo(), np.zeros(256, np.uint32)
        self._check(self._lib.polaris_hip_read_exposure(self._h, C.byref(info), hist.ctypes.data), self._h)
        return {**HA.exposure_info(info), "histogram": hist}

    def display_planes(self, plane, *, weight: float = 1.0, exposure: float = 1.0, block_y: int = 0, block_h: int | None = None, rgba=None,
                       prev_log2E=None, **fields) -> tuple[np.ndarray, np.ndarray, dict]:
        """polaris_hip_display_planes: the launches of the display stage on a caller (H, W, 4) float32 plane.  fields: those of
        T.DISPLAY_DEFAULTS.  Returns (RGBA8, the 256 counts, the exposure info as read_exposure's without the histogram); rows outside
        the request come back as passed (zeros by default)."""
        (plane,), H, W = HA._planes("display_planes", plane)
        fb = HA._own("display_planes", rgba, H, W, np.uint8)
        p, info, hist = T.display_params(1, **fields), T.ExposureInfo(), np.zeros(256, np.uint32)
        prev = None if prev_log2E is None else C.byref(C.c_float(float(prev_log2E)))
        bh = H - block_y if block_h is None else block_h
        self._check(self._lib.polaris_hip_display_planes(self._h, plane.ctypes.data, W, H, int(block_y), int(bh), float(weight), float(exposure),
                                                         C.byref(p), prev, fb.ctypes.data, hist.ctypes.data, C.byref(info)), self._h)
        return fb, hist, HA.exposure_info(info)

    def read_aov(self, which: int) -> np.ndarray:
        """(H, W, 4) float32 plane of the denoiser: T.AOV_GUIDE (normal | hit distance), T.AOV_ALBEDO (albedo | leaf type bits)
        or T.AOV_DENOISED (the filtered running mean of the last denoised sync); T.AOV_TEMPORAL / T.AOV_PRIOR (temporal reuse),
        T.AOV_VARIANCE (M1 | M2 | n_eff | v) and T.AOV_PRIOR2 (variance guidance)."""
        self._commit()
        out = np.zeros((self._H, self._W, 4), dtype=np.float32)
        self._check(self._lib.polaris_hip_read_aov(self._h, int(which), out.ctypes.data, out.size), self._h)
        return out

    def read_framebuffer(self) -> np.ndarray:
        out = np.zeros((self._H, self._W, 4), dtype=np.uint8)
        self._check(self._lib.polaris_hip_read_framebuffer(self._h, out.ctypes.data, out.size), self._h)
        return out

    def tap_primary(self, req: T.BlockRequest, seed: int) -> dict:
        n = req.frame_w * req.block_h
        taps = {"primary_rays": np.zeros((n, 8), np.float32), "primary_hit": np.zeros(n, np.int32),
                "primary_wuvt": np.zeros((n, 4), np.float32), "primary_tri": np.full((n, 2), -1, np.int32)}
        self._check(self._lib.polaris_hip_tap_primary(self._h, C.byref(req), seed, taps["primary_rays"].ctypes.data,
                                                      taps["primary_hit"].ctypes.data, taps["primary_wuvt"].ctypes.data,
                                                      taps["primary_tri"].ctypes.data), self._h)
        return taps

    PROBE_BXDF, PROBE_TEXTURE, PROBE_EMISSIVE, PROBE_MATERIAL = 0, 1, 2, 3
    _PROBE_SHAPES = {0: (13, 11), 1: (2, 7), 2: (11, 9), 3: (8, 18)}

    def probe(self, kind: int, index: int, inputs) -> np.ndarray:
        """Function-level test tap (polaris_hip_probe): rows of `inputs` through the device-side BxDF / texture / light
        functions of the uploaded scene; returns one row of outputs per probe."""
        n_in, n_out = self._PROBE_SHAPES[kind]
        a = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, n_in)
        out = np.zeros((a.shape[0], n_out), np.float32)
        self._check(self._lib.polaris_hip_probe(self._h, kind, index, a.shape[0], a.ctypes.data, out.ctypes.data), self._h)
        return out

    def probe_intersect(self, rays, any_hit: bool = False):
        """Arbitrary rays (n, 8) = origin, maxDist, dir, unused through the selected traversal kernel
        (polaris_hip_probe_intersect).  Returns (hit (n,), wuvt (n, 4), triangle (n,))."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = r.shape[0]
        hit, wuvt, tri = np.zeros(n, np.int32), np.zeros((n, 4), np.float32), np.full(n, -1, np.int32)
        self._check(self._lib.polaris_hip_probe_intersect(self._h, r.ctypes.data, n, int(any_hit), hit.ctypes.data,
                                                          wuvt.ctypes.data, tri.ctypes.data), self._h)
        return hit, wuvt, tri

    def selftest_rcp(self, lo: float, hi: float) -> tuple[int, int, int]:
        """polaris_hip_selftest_rcp: the triangle tests' 3-instruction reciprocal against 1.0f / x over all 2^32 floats.
        Returns (mismatches with lo <= |x| <= hi, mismatches outside, bit pattern of one mismatch inside)."""
        a, b, smp = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self._lib.polaris_hip_selftest_rcp(self._h, lo, hi, C.byref(a), C.byref(b), C.byref(smp)), self._h)
        return a.value, b.value, smp.value

    def selftest_builtins(self, fn: int, first: int = 0, count: int | None = None, *, results: bool = False) -> np.ndarray:
        """polaris_hip_selftest_builtins: built-in fn of polaris_math.h on the device over inputs [first, first + count).
        Returns the (chunks, 2) uint64 fingerprints (inside / outside the domain), or with results=True the (count,) result bits."""
        if count is None:
            count = T.builtin_inputs(fn) - first
        fp = None if results else np.zeros((-(-count // T.BUILTIN_CHUNK), 2), np.uint64)
        raw = np.zeros(count, np.uint32) if results else None
        self._check(self._lib.polaris_hip_selftest_builtins(self._h, int(fn), int(first), int(count), None if fp is None else fp.ctypes.data,
                                                            None if raw is None else raw.ctypes.data), self._h)
        return raw if results else fp

    def denoise_planes(self, acc, guide, albedo, *, weight: float, exposure: float, block_y: int = 0, block_h: int | None = None,
                       denoised=None, rgba=None, iterations: int = 4, normal_power_log2: int = 5, sigma_depth: float = 0.1,
                       sigma_luminance: float = 4.0) -> tuple[np.ndarray, np.ndarray]:
        """polaris_hip_denoise_planes: the launches of a denoised sync on caller (H, W, 4) float32 planes.  Returns (DENOISED plane,
        RGBA8 frame); rows outside [block_y, block_y + block_h) come back as `denoised` / `rgba` gave them (zeros by default)."""
        (acc, guide, albedo), H, W = HA._planes("denoise_planes", acc, guide, albedo)
        out, fb = HA._own("denoise_planes", denoised, H, W, np.float32), HA._own("denoise_planes", rgba, H, W, np.uint8)
        p = T.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_luminance)
        bh = H - block_y if block_h is None else block_h
        self._check(self._lib.polaris_hip_denoise_planes(self._h, acc.ctypes.data, guide.ctypes.data, albedo.ctypes.data, W, H, int(block_y),
                                                         int(bh), float(weight), float(exposure), C.byref(p), out.ctypes.data,
                                                         fb.ctypes.data), self._h)
        return out, fb

    def variance_planes(self, acc, guide, albedo, *, samples: int, exposure: float = 1.0, block_y: int = 0, block_h: int | None = None,
                        variance=None, denoised=None, rgba=None, iterations: int = 4, normal_power_log2: int = 5, sigma_depth: float = 0.1,
                        sigma_luminance: float = 4.0, sigma_variance: float = 8.0, min_samples: int = 8) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """polaris_hip_variance_planes: the launches of a variance sync on caller (H, W, 4) float32 planes (acc: rgb | sum L^2 of
        `samples` samples).  Returns (VARIANCE, DENOISED, RGBA8); rows outside the request come back as passed (zeros by default)."""
        (acc, guide, albedo), H, W = HA._planes("variance_planes", acc, guide, albedo)
        var, out, fb = (HA._own("variance_planes", a, H, W, dt) for a, dt in ((variance, np.float32), (denoised, np.float32), (rgba, np.uint8)))
        p = T.denoise_params(iterations, normal_power_log2, sigma_depth, sigma_luminance)
        v = T.variance_params(sigma_variance, min_samples)
        bh = H - block_y if block_h is None else block_h
        self._check(self._lib.polaris_hip_variance_planes(self._h, acc.ctypes.data, guide.ctypes.data, albedo.ctypes.data, W, H, int(block_y),
                                                          int(bh), int(samples), float(exposure), C.byref(p), C.byref(v), var.ctypes.data,
                                                          out.ctypes.data, fb.ctypes.data), self._h)
        return var, out, fb

    def reproject_planes(self, history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, *,
                         max_history: int = 32, normal_threshold: float = 0.9, depth_threshold: float = 0.1) -> np.ndarray:
        """polaris_hip_reproject_planes: the PRIOR plane ((H, W, 4) float32, h rgb | m) of the history planes seen under
        (prev_eye, prev_frustum), reprojected onto the G-buffer (guide, albedo) under (eye, frustum), on the device."""
        return self._reproject_planes("reproject_planes", history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum,
                                      (max_history, normal_threshold, depth_threshold))

    def _reproject_planes(self, name, *args, **groups):
        """One of the three polaris_hip_reproject*_planes entries through the marshalling of their CPU restatements (host_api._reproject:
        ValueError on shapes no entry takes; what the library refuses is a TracerError)."""
        entry = getattr(self._lib, "polaris_hip_" + name)
        return HA._reproject(name, lambda *a: self._check(entry(self._h, *a), self._h), *args, **groups)

    def reproject_motion_planes(self, history, prev_guide, prev_albedo, prev_instance, prev_eye, prev_frustum, guide, albedo, instance, eye,
                                frustum, prev_inv_transforms, inv_transforms, *, history_variance=None, max_history: int = 32,
                                normal_threshold: float = 0.9, depth_threshold: float = 0.1):
        """polaris_hip_reproject_motion_planes: reproject_planes with object motion -- the two (H, W) uint32 INSTANCE planes and the two
        (n, 16) inv_transform tables (column major, as MESH_INSTANCE) the history and the current frame were seen with.  Returns the
        PRIOR plane, or (PRIOR, PRIOR2) when the history's VARIANCE plane is given."""
        return self._reproject_planes("reproject_motion_planes", history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum,
                                      (max_history, normal_threshold, depth_threshold), history_variance=history_variance,
                                      instances=(prev_instance, instance), tables=(prev_inv_transforms, inv_transforms))

    def read_instance_plane(self) -> np.ndarray:
        """(H, W) uint32 INSTANCE plane of the first-hit G-buffer (polaris_hip_read_instance_plane; option "object_motion" with temporal
        reuse on): the mesh-instance index of every pixel's first hit, 0xFFFFFFFF for a miss."""
        self._commit()
        out = np.zeros((self._H, self._W), dtype=np.uint32)
        self._check(self._lib.polaris_hip_read_instance_plane(self._h, out.ctypes.data, out.size), self._h)
        return out

    def reproject_deform_planes(self, history, prev_guide, prev_albedo, prev_instance, prev_eye, prev_frustum, guide, albedo, instance, eye,
                                frustum, prev_inv_transforms, inv_transforms, hit, vertices, prev_vertices, *, history_variance=None,
                                max_history: int = 32, normal_threshold: float = 0.9, depth_threshold: float = 0.1):
        """polaris_hip_reproject_deform_planes: reproject_motion_planes with vertex motion -- the current (H, W, 4) uint32 HIT plane and
        the (3 NT, 4) vertices of the scene now and as the history saw them.  Returns the PRIOR plane, or (PRIOR, PRIOR2) when the
        history's VARIANCE plane is given.  (Null vertices or no triangle are passed on: the library refuses them.)"""
        return self._reproject_planes("reproject_deform_planes", history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum,
                                      (max_history, normal_threshold, depth_threshold), history_variance=history_variance,
                                      instances=(prev_instance, instance), tables=(prev_inv_transforms, inv_transforms),
                                      deform=(hit, vertices, prev_vertices))

    def read_hit_plane(self) -> np.ndarray:
        """(H, W, 4) uint32 HIT plane of the first-hit G-buffer (polaris_hip_read_hit_plane; option "vertex_motion" in effect): the scene
        triangle of every pixel's first hit | the bits of its barycentric u | of v | 0; 0xFFFFFFFF | 0 | 0 | 0 for a miss."""
        self._commit()
        out = np.zeros((self._H, self._W, 4), dtype=np.uint32)
        self._check(self._lib.polaris_hip_read_hit_plane(self._h, out.ctypes.data, out.size), self._h)
        return out

    def update_instances(self, inv, boxes, emissives=None) -> None:
        """Move the uploaded scene's mesh instances in place (polaris_hip_update_instances): inv (NI, 16) column-major
        inverse matrices, boxes (NI, 6) world-space min.xyz, max.xyz, emissives the scene's emissive array with new transform / area
        (None: unchanged) -- scenes.instance_update_args(scene) makes the triple.  The scene must have been uploaded with the option
        "instance_update" on.  Queued state changes are committed first, as by Trace."""
        self._commit()
        u, keep = T.instance_update(inv, boxes, emissives)
        self._check(self._lib.polaris_hip_update_instances(self._h, C.byref(u)), self._h)
        del keep

    def update_vertices(self, vertices, boxes, normals=None, inv=None, emissives=None) -> None:
        """Deform the uploaded scene's meshes in place (polaris_hip_update_vertices): vertices (3 NT, 4) as the scene's,
        boxes (NI, 6) world-space min.xyz, max.xyz of the deformed instances, normals (3 NT, 4) (None: unchanged), inv (NI, 16)
        column-major inverse matrices (None: unchanged), emissives the scene's emissive array with new transform / area (None:
        unchanged) -- scenes.vertex_update_args(scene) makes the tuple.  The scene must have been uploaded with the option
        "vertex_update" on.  Queued state changes are committed first, as by Trace."""
        self._commit()
        u, keep = T.vertex_update(vertices, boxes, normals, inv, emissives)
        self._check(self._lib.polaris_hip_update_vertices(self._h, C.byref(u)), self._h)
        del keep

    def update_materials(self, nodes, material_index=None, scene_diffuse=-1, emissive_mat_nodes=None) -> None:
        """Edit the uploaded scene's materials in place (polaris_hip_update_materials): nodes the whole new material
        node table (as many as uploaded), material_index (NT,) the triangles' roots (None: unchanged), scene_diffuse the background
        node (always taken: -1 = none), emissive_mat_nodes the new mat_node_index of every emissive (None: unchanged) --
        scenes.material_update_args(scene) makes the tuple.  No upload option.  Queued state changes are committed first, as by Trace."""
        self._commit()
        u, keep = T.material_update(nodes, material_index, scene_diffuse, emissive_mat_nodes)
        self._check(self._lib.polaris_hip_update_materials(self._h, C.byref(u)), self._h)
        del keep

    def update_texture(self, index: int, texels) -> None:
        """Replace the texels of texture `index` in place (polaris_hip_update_texture): same format and size as uploaded."""
        self._commit()
        t = np.ascontiguousarray(texels)
        self._check(self._lib.polaris_hip_update_texture(self._h, int(index), t.ctypes.data, t.nbytes), self._h)

    def read_triangle_records(self) -> np.ndarray:
        """The triangle records of the uploaded scene as the device holds them, one per slot (POLARIS_REC_TRIS; test tap): an array
        of ctypes_api.TRI_RECORD."""
        self._commit()
        tris = np.zeros(int(self.read_shading_record()[3]), T.TRI_RECORD)
        self._check(self._lib.polaris_hip_read_scene_records(self._h, T.REC_TRIS, tris.ctypes.data, max(tris.nbytes, 1)), self._h)
        return tris

    def read_shading_record(self) -> tuple[int, int, int, int]:
        """(tri_bits, emit_classes, background node, triangle slots) of the uploaded scene: POLARIS_REC_SHADING."""
        self._commit()
        rec = np.zeros(4, np.uint32)
        self._check(self._lib.polaris_hip_read_scene_records(self._h, T.REC_SHADING, rec.ctypes.data, rec.nbytes), self._h)
        return int(rec[0]), int(rec[1]), int(rec[2].astype(np.int32)), int(rec[3])

    def read_scene_records(self) -> tuple[np.ndarray, np.ndarray]:
        """(pair records, instance records) of the uploaded scene as the device holds them (polaris_hip_read_scene_records; test tap):
        arrays of ctypes_api.PAIR_RECORD and INST_RECORD."""
        self._commit()
        counts = self.scene_counts()
        pairs, insts = np.zeros(int(counts[0]), T.PAIR_RECORD), np.zeros(int(counts[1]), T.INST_RECORD)
        self._check(self._lib.polaris_hip_read_scene_records(self._h, T.REC_PAIRS, pairs.ctypes.data, max(pairs.nbytes, 1)), self._h)
        self._check(self._lib.polaris_hip_read_scene_records(self._h, T.REC_INSTS, insts.ctypes.data, max(insts.nbytes, 1)), self._h)
        return pairs, insts

    def scene_counts(self) -> tuple[int, int, int, int]:
        """(pair records, instance records, device allocations the scene owns, bytes in them): POLARIS_REC_COUNTS."""
        counts = np.zeros(4, np.uint64)
        self._check(self._lib.polaris_hip_read_scene_records(self._h, T.REC_COUNTS, counts.ctypes.data, counts.nbytes), self._h)
        return tuple(int(v) for v in counts)

    def kernel_ms(self, name: str) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        self._check(self._lib.polaris_hip_kernel_ms(self._h, name.encode(), C.byref(ms), C.byref(n)), self._h)
        return ms.value, n.value

    def kernel_symbol(self, name: str) -> str:
        """The kernel symbol the named timer last bracketed (polaris_hip_kernel_symbol)."""
        buf = C.create_string_buffer(128)
        self._check(self._lib.polaris_hip_kernel_symbol(self._h, name.encode(), buf), self._h)
        return buf.value.decode()

    SHADE_TIMERS = ("shade_first", "shade_sort", "shade_plain", "shade_wave")

    def shade_counts(self, bounces: int) -> list[dict]:
        """Per bounce of the last Trace: shaded hits / misses / emitter hits and the shade timer the step ran under."""
        a = (C.c_uint64 * (4 * T.MAX_BOUNCES))()
        self._check(self._lib.polaris_hip_shade_counts(self._h, a, len(a)), self._h)
        return [{"hits": int(a[4 * b]), "misses": int(a[4 * b + 1]), "emitters": int(a[4 * b + 2]), "timer": self.SHADE_TIMERS[int(a[4 * b + 3])]}
                for b in range(bounces)]

    def export_block(self, req: T.BlockRequest, device_ptr: int) -> None:
        self._check(self._lib.polaris_hip_export_block(self._h, C.byref(req), C.c_void_p(device_ptr)), self._h)

    def reset_frame(self) -> None:
        """The pipeline's Reset stage on its own (tracer/opencl/tracer.go:208-213)."""
        self._check(self._lib.polaris_hip_reset_frame(self._h), self._h)

    def merge_device(self, device_ptr: int, req: T.BlockRequest) -> None:
        self._check(self._lib.polaris_hip_merge_device(self._h, C.c_void_p(device_ptr), C.byref(req)), self._h)

    # ---- cross-process merge: peer reads over HIP IPC (include/polaris_hip.h) ------------------------
    def ipc_export(self, depth: int = 3) -> bytes:
        """The trace accumulator becomes a ring of `depth` buffers; returns the PolarisIpcExport blob a peer PROCESS opens."""
        x = T.IpcExport()
        self._check(self._lib.polaris_hip_ipc_export(self._h, depth, C.byref(x)), self._h)
        return bytes(x)

    def ipc_open(self, blob: bytes) -> int:
        """Map another process's ring (its ipc_export blob) on this tracer's device; returns the peer handle."""
        x = T.IpcExport.from_buffer_copy(blob)
        p = C.c_void_p()
        self._check(self._lib.polaris_hip_ipc_open(self._h, C.byref(x), C.byref(p)), self._h)
        return p.value

    def ipc_close(self, peer: int) -> None:
        self._check(self._lib.polaris_hip_ipc_close(self._h, C.c_void_p(peer)), self._h)

    def merge_ipc(self, peer: int, slot: int, req: T.BlockRequest) -> None:
        """MergeOutput from a peer process: rows of `req` of the peer's ring slot, read through the IPC mapping."""
        self._check(self._lib.polaris_hip_merge_ipc(self._h, C.c_void_p(peer), slot, C.byref(req)), self._h)

    def merge_slot(self, other: "HipTracer", slot: int, req: T.BlockRequest) -> None:
        """MergeOutput from ring slot `slot` of a tracer of this process (the primary's own block, merged one frame late)."""
        self._check(self._lib.polaris_hip_merge_slot(self._h, other._h, slot, C.byref(req)), self._h)

    def peer_info(self, peer: int) -> dict:
        """What a mapped peer ring really is (polaris_hip_peer_info): the exporter's GPU by PCI bus id, whether it is this tracer's own
        GPU, and the merge branch that follows from it ("ipc-local" / "ipc-peer" / "ipc-unknown"; "ipc-staged" where the merges go
        through the staging strip: no peer access to the ring's GPU, or option ipc_staged)."""
        i = T.PeerInfo()
        self._check(self._lib.polaris_hip_peer_info(C.c_void_p(peer), C.byref(i)), None)
        same = int(i.same_device)
        return {"pid": int(i.pid), "exporter_device": int(i.exporter_device), "pci_bus_id": i.pci_bus_id.decode(errors="replace"),
                "local_device": int(i.local_device), "same_device": same, "can_access_peer": int(i.can_access_peer), "depth": int(i.depth),
                "has_events": int(i.has_events), "staged": int(i.staged),
                "branch": "ipc-staged" if i.staged else ("ipc-local" if same == 1 else ("ipc-peer" if same == 0 else "ipc-unknown"))}

    def merge_counts(self) -> dict:
        """How many merges onto this tracer took which branch since it was created (polaris_hip_merge_counts)."""
        a = (C.c_uint64 * len(T.MERGE_BRANCHES))()
        self._check(self._lib.polaris_hip_merge_counts(self._h, a), self._h)
        return {name: int(a[k]) for k, name in enumerate(T.MERGE_BRANCHES)}

    def device_identity(self) -> dict:
        """Which physical GPU this tracer runs on (polaris_hip_device_identity of its device index)."""
        return T.device_identity(self._device)

    def trace_slot(self) -> int:
        s = C.c_uint32()
        self._check(self._lib.polaris_hip_trace_slot(self._h, C.byref(s)), self._h)
        return int(s.value)

    @property
    def device_name(self) -> str:
        return self._name

    # ---- internals ---------------------------------------------------------------------------
    def _commit(self) -> float:
        if not self._changes:
            return 0.0
        t0 = time.perf_counter()
        for change, data in list(self._changes.items()):
            if change == ChangeType.FrameDimensions:
                self._W, self._H = int(data[0]), int(data[1])
                self._check(self._lib.polaris_hip_resize(self._h, self._W, self._H), self._h)
            elif change == ChangeType.SceneData:
                view = T.scene_view(data)
                self._check(self._lib.polaris_hip_upload_scene(self._h, C.byref(view)), self._h)
            elif change == ChangeType.CameraData:
                eye = np.ascontiguousarray(data.eye, dtype=np.float32)
                fr = np.ascontiguousarray(data.frustum, dtype=np.float32)
                self._check(self._lib.polaris_hip_set_camera(self._h, eye.ctypes.data_as(C.POINTER(C.c_float)),
                                                             fr.ctypes.data_as(C.POINTER(C.c_float))), self._h)
                self._camera = data
                self._shutter = None         # (set_camera switched the shutter off: its close camera belonged to the camera that went)
                if self._lens is not None:   # (set_camera leaves the lens vectors alone: they follow the new frustum here)
                    self._apply_lens()
                if self._projection is not None:   # (... and the projection's basis)
                    self._apply_projection()
            else:
                raise TracerError(2, f"unsupported change type {change}")
        self._changes.clear()
        self._stats.UpdateTime = time.perf_counter() - t0
        return self._stats.UpdateTime

    def _check(self, rc: int, h) -> None:
        if rc == 0:
            return
        msg = self._lib.polaris_hip_last_error(h if h else None)
        msg = msg.decode() if msg else ""
        if rc == E_NO_SCENE_DATA:
            raise ErrNoSceneData(rc, msg)
        raise TracerError(rc, msg)
