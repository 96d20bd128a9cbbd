"""ctypes mirrors of include/polaris_types.h and the loader for the C-ABI library.

The numpy dtypes below are byte-for-byte the structs of include/polaris_types.h, which are in
turn the reference's device layouts (asset/scene/optimized_scene.go:25-190, CL/types.cl:4-187).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libpolaris_hip.so")

MAX_BOUNCES = 32

# ---- numpy structured dtypes (scene arrays) -------------------------------------------------
BVH_NODE = np.dtype([("min", "<f4", 3), ("ldata", "<i4"), ("max", "<f4", 3), ("rdata", "<i4")])
MESH_INSTANCE = np.dtype([("mesh_index", "<u4"), ("bvh_root", "<u4"), ("reserved", "<u4", 2),
                          ("inv_transform", "<f4", 16)])
MATERIAL_NODE = np.dtype([("type", "<u4"), ("left_child", "<u4"), ("right_child", "<i4"), ("tex", "<i4"),
                          ("k", "<f4", 4), ("t", "<f4", 4), ("int_ior", "<f4"), ("ext_ior", "<f4"),
                          ("scale", "<f4"), ("roughness_tex", "<i4")])
EMISSIVE = np.dtype([("transform", "<f4", 16), ("area", "<f4"), ("tri_index", "<u4"),
                     ("mat_node_index", "<u4"), ("type", "<u4")])
TEXTURE_META = np.dtype([("format", "<u4"), ("width", "<u4"), ("height", "<u4"), ("data_offset", "<u4")])
assert BVH_NODE.itemsize == 32 and MESH_INSTANCE.itemsize == 80 and MATERIAL_NODE.itemsize == 64
assert EMISSIVE.itemsize == 80 and TEXTURE_META.itemsize == 16

BXDF_INVALID, BXDF_EMISSIVE, BXDF_DIFFUSE, BXDF_CONDUCTOR = 0, 2, 4, 8
BXDF_ROUGH_CONDUCTOR, BXDF_DIELECTRIC, BXDF_ROUGH_DIELECTRIC = 16, 32, 64
OP_MIX, OP_MIX_MAP, OP_BUMP_MAP, OP_NORMAL_MAP, OP_DISPERSE = 10001, 10002, 10003, 10004, 10005
TEX_L8, TEX_L32F, TEX_RGBA8, TEX_RGBA32F = 0, 1, 2, 3
EMISSIVE_AREA, EMISSIVE_ENVIRONMENT = 0, 1


# ---- ctypes structs -------------------------------------------------------------------------
class SceneView(C.Structure):
    _fields_ = [
        ("bvh_nodes", C.c_void_p), ("num_bvh_nodes", C.c_uint32),
        ("mesh_instances", C.c_void_p), ("num_mesh_instances", C.c_uint32),
        ("material_nodes", C.c_void_p), ("num_material_nodes", C.c_uint32),
        ("emissives", C.c_void_p), ("num_emissives", C.c_uint32),
        ("texture_data", C.c_void_p), ("texture_data_bytes", C.c_uint32),
        ("texture_meta", C.c_void_p), ("num_textures", C.c_uint32),
        ("vertices", C.c_void_p), ("normals", C.c_void_p), ("uvs", C.c_void_p),
        ("material_index", C.c_void_p), ("num_triangles", C.c_uint32),
        ("scene_diffuse_mat_index", C.c_int32), ("scene_emissive_mat_index", C.c_int32),
    ]


class BlockRequest(C.Structure):
    """tracer.BlockRequest (tracer/tracer.go:6-34)."""
    _fields_ = [
        ("frame_w", C.c_uint32), ("frame_h", C.c_uint32),
        ("block_x", C.c_uint32), ("block_y", C.c_uint32), ("block_w", C.c_uint32), ("block_h", C.c_uint32),
        ("samples_per_pixel", C.c_uint32), ("num_bounces", C.c_uint32), ("min_bounces_for_rr", C.c_uint32),
        ("exposure", C.c_float), ("seed", C.c_uint32), ("accumulated_samples", C.c_uint32),
    ]


class TraceStats(C.Structure):
    _fields_ = [
        ("primary_rays", C.c_uint64), ("indirect_rays", C.c_uint64), ("occlusion_rays", C.c_uint64),
        ("shaded_hits", C.c_uint64), ("shaded_misses", C.c_uint64), ("emitter_hits", C.c_uint64),
        ("unoccluded", C.c_uint64),
        ("rays_per_bounce", C.c_uint64 * MAX_BOUNCES), ("occl_per_bounce", C.c_uint64 * MAX_BOUNCES),
        ("device_ms", C.c_double),
    ]

    def total_rays(self) -> int:
        """BASELINE.md section 3 counting rule: primary + indirect + occlusion rays traced."""
        return int(self.primary_rays + self.indirect_rays + self.occlusion_rays)

    def algorithmic_bytes(self, pixels: int, traces: int = 1, frames: int = 1) -> int:
        """compulsory stream bytes of the wavefront formulation."""
        return int(112 * self.primary_rays + 68 * self.shaded_hits + 92 * self.indirect_rays
                   + 80 * self.occlusion_rays + 44 * self.unoccluded + 60 * self.shaded_misses
                   + 24 * self.emitter_hits + 48 * pixels * traces + 16 * pixels * frames)

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in ("primary_rays", "indirect_rays", "occlusion_rays", "shaded_hits",
                                                  "shaded_misses", "emitter_hits", "unoccluded")}
        d["rays_per_bounce"] = [int(v) for v in self.rays_per_bounce]
        d["occl_per_bounce"] = [int(v) for v in self.occl_per_bounce]
        d["device_ms"] = float(self.device_ms)
        return d


IPC_MAX_DEPTH = 4


class IpcExport(C.Structure):
    """PolarisIpcExport (include/polaris_hip.h): what a tracer publishes once so that another PROCESS can map its trace
    accumulator ring.  Plain bytes: bytes(export) travels over any channel, IpcExport.from_buffer_copy(b) restores it."""
    _fields_ = [
        ("abi_version", C.c_uint32), ("depth", C.c_uint32), ("frame_w", C.c_uint32), ("frame_h", C.c_uint32),
        ("device", C.c_int32), ("pid", C.c_uint32), ("has_event", C.c_uint32), ("reserved", C.c_uint32),
        ("mem", (C.c_uint8 * 64) * IPC_MAX_DEPTH), ("event", (C.c_uint8 * 64) * IPC_MAX_DEPTH),
        ("pci_bus_id", C.c_char * 32),
    ]


assert C.sizeof(IpcExport) == 32 + 64 * IPC_MAX_DEPTH + 64 * IPC_MAX_DEPTH + 32


class DeviceIdentity(C.Structure):
    """PolarisDeviceIdentity (include/polaris_hip.h): which physical GPU a HIP device index of this process is."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("hip_index", C.c_int32), ("pci_bus_id", C.c_char * 32), ("uuid", C.c_uint8 * 16),
        ("compute_units", C.c_uint32), ("clock_mhz", C.c_uint32), ("global_mem_bytes", C.c_uint64),
        ("name", C.c_char * 64), ("gcn_arch", C.c_char * 32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)

    def as_dict(self) -> dict:
        return {"hip_index": int(self.hip_index), "pci_bus_id": self.pci_bus_id.decode(errors="replace"), "uuid": bytes(self.uuid).hex(),
                "cus": int(self.compute_units), "clock_mhz": int(self.clock_mhz), "global_mem_bytes": int(self.global_mem_bytes),
                "name": self.name.decode(errors="replace"), "gcn_arch": self.gcn_arch.decode(errors="replace")}


class PeerInfo(C.Structure):
    """PolarisPeerInfo (include/polaris_hip.h): what a mapped peer ring really is."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("pid", C.c_uint32), ("exporter_device", C.c_int32), ("local_device", C.c_int32),
        ("same_device", C.c_int32), ("can_access_peer", C.c_int32), ("depth", C.c_uint32), ("has_events", C.c_uint32),
        ("pci_bus_id", C.c_char * 32), ("staged", C.c_int32), ("reserved", C.c_int32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(DeviceIdentity) == 168 and C.sizeof(PeerInfo) == 72


class DenoiseParams(C.Structure):
    """PolarisDenoiseParams (include/polaris_hip.h): the edge-avoiding a-trous filter of polaris_hip_sync_framebuffer."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32),
        ("sigma_depth", C.c_float), ("sigma_luminance", C.c_float),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(DenoiseParams) == 20
# the settings DESIGN.md section 10 chose on the CPU restatement (include/polaris_hip.h)
DENOISE_DEFAULTS = {"iterations": 4, "normal_power_log2": 5, "sigma_depth": 0.1, "sigma_luminance": 4.0}
AOV_GUIDE, AOV_ALBEDO, AOV_DENOISED, AOV_TEMPORAL, AOV_PRIOR, AOV_VARIANCE, AOV_PRIOR2 = 0, 1, 2, 3, 4, 5, 6


class TemporalParams(C.Structure):
    """PolarisTemporalParams (include/polaris_hip.h): temporal reuse of the synced frame across camera moves."""
    _fields_ = [("struct_size", C.c_uint32), ("max_history", C.c_uint32), ("normal_threshold", C.c_float), ("depth_threshold", C.c_float)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(TemporalParams) == 16
# the settings DESIGN.md section 10b chose on the CPU restatement (include/polaris_hip.h)
TEMPORAL_DEFAULTS = {"max_history": 32, "normal_threshold": 0.9, "depth_threshold": 0.1}


def temporal_params(max_history=32, normal_threshold=0.9, depth_threshold=0.1) -> TemporalParams:
    p = TemporalParams()
    p.max_history = int(max_history)
    p.normal_threshold, p.depth_threshold = float(normal_threshold), float(depth_threshold)
    return p


class LensParams(C.Structure):
    """PolarisLensParams (include/polaris_hip.h): the thin-lens camera.  u = v = 0 is the lens OFF (the default)."""
    _fields_ = [("struct_size", C.c_uint32), ("focus_distance", C.c_float), ("axis", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(LensParams) == 44


def lens_params(focus_distance=0.0, axis=(0.0, 0.0, 0.0), u=(0.0, 0.0, 0.0), v=(0.0, 0.0, 0.0)) -> LensParams:
    p = LensParams()
    p.focus_distance = float(focus_distance)
    for name, vec in (("axis", axis), ("u", u), ("v", v)):
        setattr(p, name, (C.c_float * 3)(*[float(x) for x in vec]))
    return p


def lens_from_frustum(frustum, radius):
    """(axis, u, v) of a round lens of this radius facing the way the frustum looks: axis = normalize(TL + TR + BL + BR),
    u = radius * normalize(TR - TL), v = radius * normalize(TL - BL); computed in float64, rounded to float32 once."""
    fr = np.asarray(frustum, np.float64).reshape(4, 4)[:, :3]
    tl, tr, bl, br = fr
    unit = lambda x: x / np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])  # noqa: E731  (spelled out: the host layer's C++ derives the same bits)
    return (unit(tl + tr + bl + br).astype(np.float32), (float(radius) * unit(tr - tl)).astype(np.float32),
            (float(radius) * unit(tl - bl)).astype(np.float32))


class ShutterParams(C.Structure):
    """PolarisShutterParams (include/polaris_hip.h): the camera (and, while the lens is on, the lens) at shutter close.  enabled = 0 is
    the shutter OFF (the default)."""
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("eye1", C.c_float * 3), ("frustum1", C.c_float * 16),
                ("focus_distance1", C.c_float), ("axis1", C.c_float * 3), ("u1", C.c_float * 3), ("v1", C.c_float * 3)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(ShutterParams) == 124


def shutter_params(eye1=None, frustum1=None, focus_distance1=0.0, axis1=(0.0, 0.0, 0.0), u1=(0.0, 0.0, 0.0), v1=(0.0, 0.0, 0.0)) -> ShutterParams:
    """eye1 = None: the shutter off (all else zero); else enabled = 1 with this close camera and close lens."""
    p = ShutterParams()
    if eye1 is None:
        return p
    p.enabled = 1
    p.eye1 = (C.c_float * 3)(*[float(x) for x in np.asarray(eye1).reshape(3)])
    p.frustum1 = (C.c_float * 16)(*[float(x) for x in np.asarray(frustum1).reshape(16)])
    p.focus_distance1 = float(focus_distance1)
    for name, vec in (("axis1", axis1), ("u1", u1), ("v1", v1)):
        setattr(p, name, (C.c_float * 3)(*[float(x) for x in vec]))
    return p


PROJECTION_PERSPECTIVE, PROJECTION_ORTHOGRAPHIC, PROJECTION_EQUIRECTANGULAR = 0, 1, 2
PROJECTION_KINDS = {"perspective": PROJECTION_PERSPECTIVE, "orthographic": PROJECTION_ORTHOGRAPHIC, "equirect": PROJECTION_EQUIRECTANGULAR}


class ProjectionParams(C.Structure):
    """PolarisProjectionParams (include/polaris_hip.h): the orthographic or the equirectangular camera.  kind = 0 is the projection OFF
    (the default): the perspective frustum of polaris_hip_set_camera."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("axis", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("half_width", C.c_float), ("half_height", C.c_float), ("lon_range", C.c_float), ("lat_range", C.c_float)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(ProjectionParams) == 60


def projection_params(kind=PROJECTION_PERSPECTIVE, axis=(0.0, 0.0, 0.0), right=(0.0, 0.0, 0.0), up=(0.0, 0.0, 0.0), half_width=0.0, half_height=0.0,
                      lon_range=0.0, lat_range=0.0) -> ProjectionParams:
    p = ProjectionParams()
    p.kind = int(kind)
    for name, vec in (("axis", axis), ("right", right), ("up", up)):
        setattr(p, name, (C.c_float * 3)(*[float(x) for x in vec]))
    p.half_width, p.half_height, p.lon_range, p.lat_range = float(half_width), float(half_height), float(lon_range), float(lat_range)
    return p


def projection_from_frustum(frustum):
    """(axis, right, up, aspect) of the view basis a perspective frustum looks through: axis = normalize(TL + TR + BL + BR),
    right = normalize(TR - TL), up = normalize(TL - BL) made orthogonal to axis, aspect = |TR - TL| / |TL - BL|; computed in float64,
    the vectors rounded to float32 once."""
    fr = np.asarray(frustum, np.float64).reshape(4, 4)[:, :3]
    tl, tr, bl, br = fr
    length = lambda x: np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])  # noqa: E731  (spelled out: the host layer's C++ derives the same bits)
    axis = (tl + tr + bl + br) / length(tl + tr + bl + br)
    right = (tr - tl) / length(tr - tl)
    up = (tl - bl) / length(tl - bl)
    up = up - axis * ((up[0] * axis[0] + up[1] * axis[1]) + up[2] * axis[2])
    up = up / length(up)
    return axis.astype(np.float32), right.astype(np.float32), up.astype(np.float32), float(length(tr - tl) / length(tl - bl))


def projection_for(kind, frustum, height=None, lon_range=2.0 * np.pi, lat_range=np.pi) -> ProjectionParams:
    """The projection `kind` (a PROJECTION_* number) looking the way the frustum looks.  ORTHOGRAPHIC: a window `height` world units
    high, as wide as the frustum's aspect makes it.  EQUIRECTANGULAR: lon_range x lat_range radians."""
    if kind == PROJECTION_PERSPECTIVE:
        return projection_params()
    axis, right, up, aspect = projection_from_frustum(frustum)
    if kind == PROJECTION_ORTHOGRAPHIC:
        if height is None:
            raise ValueError("an orthographic projection needs the height of its window")
        half_height = float(height) / 2.0
        return projection_params(kind, axis, right, up, half_width=half_height * aspect, half_height=half_height)
    return projection_params(kind, axis, right, up, lon_range=lon_range, lat_range=lat_range)


class VarianceParams(C.Structure):
    """PolarisVarianceParams (include/polaris_hip.h): variance-guided denoising from per-pixel luminance moments."""
    _fields_ = [("struct_size", C.c_uint32), ("sigma_variance", C.c_float), ("min_samples", C.c_uint32)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(VarianceParams) == 12
# the settings DESIGN.md section 10c chose on the CPU restatement (profiles/variance_quality.txt)
VARIANCE_DEFAULTS = {"sigma_variance": 8.0, "min_samples": 8}


TONE_REINHARD, TONE_REINHARD_WHITE, TONE_ACES, TONE_HABLE = 0, 1, 2, 3
TONE_OPERATORS = {"reinhard": TONE_REINHARD, "reinhard-white": TONE_REINHARD_WHITE, "aces": TONE_ACES, "hable": TONE_HABLE}


class DisplayParams(C.Structure):
    """PolarisDisplayParams (include/polaris_hip.h): the display transform of SyncFramebuffer -- auto-exposure, tone curve, transfer."""
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("tone_operator", C.c_uint32), ("srgb", C.c_uint32), ("white", C.c_float),
                ("auto_exposure", C.c_uint32), ("key", C.c_float), ("compensation_ev", C.c_float), ("low_permille", C.c_uint32),
                ("high_permille", C.c_uint32), ("min_ev", C.c_float), ("max_ev", C.c_float), ("adapt", C.c_float)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(DisplayParams)


class ExposureInfo(C.Structure):
    """PolarisExposureInfo (include/polaris_hip.h): what the last sync with auto-exposure on metered."""
    _fields_ = [("struct_size", C.c_uint32), ("valid", C.c_uint32), ("n_metered", C.c_uint64), ("avg", C.c_float), ("log2E", C.c_float),
                ("E", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(ExposureInfo)


assert C.sizeof(DisplayParams) == 52 and C.sizeof(ExposureInfo) == 32
# the suggested settings: middle grey, the window between the median and the 95th percentile, snap
DISPLAY_DEFAULTS = {"tone_operator": TONE_REINHARD, "srgb": 0, "white": 4.0, "auto_exposure": 0, "key": 0.18, "compensation_ev": 0.0,
                    "low_permille": 500, "high_permille": 950, "min_ev": -16.0, "max_ev": 16.0, "adapt": 1.0}


def display_params(enabled=1, **kw) -> DisplayParams:
    """DisplayParams with DISPLAY_DEFAULTS for the fields not given (tone_operator: a TONE_* number or a TONE_OPERATORS name)."""
    unknown = set(kw) - set(DISPLAY_DEFAULTS)
    if unknown:
        raise TypeError(f"display_params: unknown fields {sorted(unknown)}")
    f = dict(DISPLAY_DEFAULTS, **kw)
    p = DisplayParams()
    p.enabled = int(enabled)
    p.tone_operator = TONE_OPERATORS[f["tone_operator"]] if isinstance(f["tone_operator"], str) else int(f["tone_operator"])
    p.srgb, p.auto_exposure = int(f["srgb"]), int(f["auto_exposure"])
    p.low_permille, p.high_permille = int(f["low_permille"]), int(f["high_permille"])
    for name in ("white", "key", "compensation_ev", "min_ev", "max_ev", "adapt"):
        setattr(p, name, float(f[name]))
    return p


class BloomParams(C.Structure):
    """PolarisBloomParams (include/polaris_hip.h): the bloom of the display transform -- a bright-pass pyramid added before the tone curve."""
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("levels", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float),
                ("intensity", C.c_float), ("karis", C.c_uint32)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(BloomParams)


assert C.sizeof(BloomParams) == 28
# the suggested settings, chosen on the Cornell boxes with the CPU restatement
BLOOM_DEFAULTS = {"levels": 5, "threshold": 1.0, "knee": 0.5, "intensity": 0.25, "karis": 1}


def bloom_params(enabled=1, **kw) -> BloomParams:
    """BloomParams with BLOOM_DEFAULTS for the fields not given."""
    unknown = set(kw) - set(BLOOM_DEFAULTS)
    if unknown:
        raise TypeError(f"bloom_params: unknown fields {sorted(unknown)}")
    f = dict(BLOOM_DEFAULTS, **kw)
    p = BloomParams()
    p.enabled, p.levels, p.karis = int(enabled), int(f["levels"]), int(f["karis"])
    p.threshold, p.knee, p.intensity = float(f["threshold"]), float(f["knee"]), float(f["intensity"])
    return p


def variance_params(sigma_variance=8.0, min_samples=8) -> VarianceParams:
    p = VarianceParams()
    p.sigma_variance, p.min_samples = float(sigma_variance), int(min_samples)
    return p

# polaris_hip_selftest_builtins / polaris_oracle_builtins: the probed built-ins (enum PbFn, polaris_amd/csrc/builtin_probe.h)
BUILTINS_UNARY = ("sqrt", "rcp", "floor", "fabs", "sign", "sin", "cos", "atan", "acos", "log", "exp", "pow_gamma", "convert_float_uint",
                  "tonemap")
BUILTINS_MULTI = ("atan2", "pow", "divide", "min", "max", "fmin", "fmax", "clamp", "mix")
BUILTINS = {name: fn for fn, name in enumerate(BUILTINS_UNARY + BUILTINS_MULTI)}
BUILTIN_CHUNK = 1 << 20
BUILTIN_EDGES, BUILTIN_DRAWS = 24, 1 << 28
SELFTEST_MAX_RESULTS = 1 << 24   # POLARIS_SELFTEST_MAX_RESULTS_LOG2


def builtin_inputs(fn: int) -> int:
    """Inputs of built-in fn: every 2^32 bit pattern (unary) or the 24^3 edge grid and 2^28 draws."""
    return 1 << 32 if fn < len(BUILTINS_UNARY) else BUILTIN_EDGES ** 3 + BUILTIN_DRAWS


def denoise_params(iterations=4, normal_power_log2=5, sigma_depth=0.1, sigma_luminance=4.0) -> DenoiseParams:
    p = DenoiseParams()
    p.iterations, p.normal_power_log2 = int(iterations), int(normal_power_log2)
    p.sigma_depth, p.sigma_luminance = float(sigma_depth), float(sigma_luminance)
    return p
MERGE_BRANCHES = ("local", "peer-access", "staged", "ipc-local", "ipc-peer", "ipc-unknown", "device-strip", "ipc-staged")   # POLARIS_MERGE_* (include/polaris_hip.h)


def device_identity(index: int) -> dict:
    """polaris_hip_device_identity as a dict (hip_index, pci_bus_id, uuid hex, cus, clock_mhz, global_mem_bytes, name, gcn_arch)."""
    lib = load_library()
    d = DeviceIdentity()
    rc = lib.polaris_hip_device_identity(int(index), C.byref(d))
    if rc:
        msg = lib.polaris_hip_last_error(None)
        raise RuntimeError(f"polaris_hip_device_identity({index}) failed with {rc}: {msg.decode() if msg else ''}")
    return d.as_dict()


def can_access_peer(device: int, peer: int) -> int:
    """hipDeviceCanAccessPeer(device, peer) for two device indices of this process (0 for device == peer)."""
    lib = load_library()
    can = C.c_int(0)
    rc = lib.polaris_hip_can_access_peer(int(device), int(peer), C.byref(can))
    if rc:
        msg = lib.polaris_hip_last_error(None)
        raise RuntimeError(f"polaris_hip_can_access_peer({device}, {peer}) failed with {rc}: {msg.decode() if msg else ''}")
    return int(can.value)


class BvhBuildInput(C.Structure):
    """PolarisBvhBuildInput (include/polaris_hip.h): what polaris_hip_build_bvh builds the two-level BVH from."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("vertices", C.c_void_p), ("num_triangles", C.c_uint32),
        ("mesh_first_tri", C.c_void_p), ("mesh_num_tris", C.c_void_p), ("num_meshes", C.c_uint32),
        ("instance_boxes", C.c_void_p), ("instance_mesh", C.c_void_p), ("num_instances", C.c_uint32),
        ("max_leaf_tris", C.c_uint32), ("algorithm", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)   # (the library refuses another layout: ABI 5)


BVH_SAH, BVH_LBVH = 0, 1   # PolarisBvhBuildInput.algorithm


class InstanceUpdate(C.Structure):
    """PolarisInstanceUpdate (include/polaris_hip.h): what polaris_hip_update_instances moves the uploaded scene's instances to."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_mesh_instances", C.c_uint32),
        ("inv_transforms", C.c_void_p), ("instance_boxes", C.c_void_p),
        ("emissives", C.c_void_p), ("num_emissives", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(InstanceUpdate) == 40
REC_PAIRS, REC_INSTS, REC_COUNTS = 0, 1, 2   # polaris_hip_read_scene_records
PAIR_RECORD = np.dtype([("lo0", "<f4", 3), ("ref0", "<i4"), ("hi0", "<f4", 3), ("cull0", "<f4"),
                        ("lo1", "<f4", 3), ("ref1", "<i4"), ("hi1", "<f4", 3), ("cull1", "<f4")])
INST_RECORD = np.dtype([("r0", "<f4", 4), ("r1", "<f4", 4), ("r2", "<f4", 4), ("root_ref", "<i4"), ("rank", "<u4"), ("pad", "<u4", 2)])
assert PAIR_RECORD.itemsize == 64 and INST_RECORD.itemsize == 64


def instance_update(inv, boxes, emissives=None):
    """An InstanceUpdate over the given arrays, and the arrays it borrows (keep them alive while it is used)."""
    inv = np.ascontiguousarray(inv, dtype=np.float32).reshape(-1, 16)
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    u = InstanceUpdate()
    u.num_mesh_instances = len(inv)
    u.inv_transforms, u.instance_boxes = inv.ctypes.data, boxes.ctypes.data
    keep = [inv, boxes]
    if emissives is not None:
        em = np.ascontiguousarray(emissives, dtype=EMISSIVE)
        u.emissives, u.num_emissives = (em.ctypes.data if em.size else None), len(em)
        keep.append(em)
    return u, keep


class VertexUpdate(C.Structure):
    """PolarisVertexUpdate (include/polaris_hip.h): what polaris_hip_update_vertices deforms the uploaded scene's meshes to."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_triangles", C.c_uint32),
        ("vertices", C.c_void_p), ("normals", C.c_void_p),
        ("num_mesh_instances", C.c_uint32), ("instance_boxes", C.c_void_p), ("inv_transforms", C.c_void_p),
        ("emissives", C.c_void_p), ("num_emissives", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(VertexUpdate) == 64


def vertex_update(vertices, boxes, normals=None, inv=None, emissives=None):
    """A VertexUpdate over the given arrays, and the arrays it borrows (keep them alive while it is used)."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 4)
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    u = VertexUpdate()
    u.num_triangles, u.num_mesh_instances = len(vertices) // 3, len(boxes)
    u.vertices, u.instance_boxes = vertices.ctypes.data, boxes.ctypes.data
    keep = [vertices, boxes]
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 4)
        assert len(normals) == len(vertices)
        u.normals = normals.ctypes.data
        keep.append(normals)
    if inv is not None:
        inv = np.ascontiguousarray(inv, dtype=np.float32).reshape(-1, 16)
        assert len(inv) == len(boxes)
        u.inv_transforms = inv.ctypes.data
        keep.append(inv)
    if emissives is not None:
        em = np.ascontiguousarray(emissives, dtype=EMISSIVE)
        u.emissives, u.num_emissives = (em.ctypes.data if em.size else None), len(em)
        keep.append(em)
    return u, keep


class MaterialUpdate(C.Structure):
    """PolarisMaterialUpdate (include/polaris_hip.h): the materials polaris_hip_update_materials gives the uploaded scene."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_material_nodes", C.c_uint32), ("material_nodes", C.c_void_p),
        ("num_triangles", C.c_uint32), ("material_index", C.c_void_p),
        ("scene_diffuse_mat_index", C.c_int32), ("emissive_mat_nodes", C.c_void_p), ("num_emissives", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(self)


assert C.sizeof(MaterialUpdate) == 56
REC_TRIS, REC_SHADING = 3, 4   # polaris_hip_read_scene_records
TRI_RECORD = np.dtype([("v0", "<f4", 3), ("rank", "<u4"), ("e1", "<f4", 3), ("orig", "<u4"), ("e2", "<f4", 3), ("word", "<u4")])
assert TRI_RECORD.itemsize == 48


def material_update(nodes, material_index=None, scene_diffuse=-1, emissive_mat_nodes=None):
    """A MaterialUpdate over the given arrays, and the arrays it borrows (keep them alive while it is used)."""
    nodes = np.ascontiguousarray(nodes, dtype=MATERIAL_NODE)
    u = MaterialUpdate()
    u.num_material_nodes, u.material_nodes = len(nodes), (nodes.ctypes.data if nodes.size else None)
    u.scene_diffuse_mat_index = int(scene_diffuse)
    keep = [nodes]
    if material_index is not None:
        mi = np.ascontiguousarray(material_index, dtype=np.uint32).reshape(-1)
        u.num_triangles, u.material_index = len(mi), mi.ctypes.data
        keep.append(mi)
    if emissive_mat_nodes is not None:
        em = np.ascontiguousarray(emissive_mat_nodes, dtype=np.uint32).reshape(-1)
        u.num_emissives, u.emissive_mat_nodes = len(em), em.ctypes.data   # (an empty list is still a list: numpy's pointer is not null)
        keep.append(em)
    return u, keep


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def scene_view(scene) -> SceneView:
    """Borrow a polaris_amd.scenes.Scene's arrays as a PolarisSceneView (arrays must stay alive)."""
    v = SceneView()
    v.bvh_nodes, v.num_bvh_nodes = _ptr(scene.bvh_nodes), len(scene.bvh_nodes)
    v.mesh_instances, v.num_mesh_instances = _ptr(scene.mesh_instances), len(scene.mesh_instances)
    v.material_nodes, v.num_material_nodes = _ptr(scene.material_nodes), len(scene.material_nodes)
    v.emissives, v.num_emissives = _ptr(scene.emissives), len(scene.emissives)
    v.texture_data, v.texture_data_bytes = _ptr(scene.texture_data), scene.texture_data.size
    v.texture_meta, v.num_textures = _ptr(scene.texture_meta), len(scene.texture_meta)
    v.vertices, v.normals, v.uvs = _ptr(scene.vertices), _ptr(scene.normals), _ptr(scene.uvs)
    v.material_index, v.num_triangles = _ptr(scene.material_index), len(scene.material_index)
    v.scene_diffuse_mat_index = int(scene.scene_diffuse_mat_index)
    v.scene_emissive_mat_index = int(scene.scene_emissive_mat_index)
    return v


# Every symbol include/polaris_hip.h declares; tests check the built library exports all of them.
C_ABI_SYMBOLS = [
    "polaris_hip_device_count", "polaris_hip_device_info", "polaris_hip_create", "polaris_hip_destroy",
    "polaris_hip_last_error", "polaris_hip_resize", "polaris_hip_upload_scene", "polaris_hip_set_camera",
    "polaris_hip_set_option", "polaris_hip_trace", "polaris_hip_merge", "polaris_hip_export_block",
    "polaris_hip_merge_device", "polaris_hip_sync_framebuffer", "polaris_hip_read_framebuffer",
    "polaris_hip_read_accumulator", "polaris_hip_tap_primary", "polaris_hip_abi_version",
    "polaris_hip_kernel_ms", "polaris_hip_reset_frame", "polaris_hip_probe", "polaris_hip_probe_intersect",
    "polaris_hip_selftest_rcp", "polaris_hip_reset_epoch", "polaris_hip_wait_reset",
    "polaris_hip_kernel_symbol", "polaris_hip_shade_counts",
    "polaris_hip_ipc_export", "polaris_hip_ipc_open", "polaris_hip_ipc_close", "polaris_hip_merge_ipc",
    "polaris_hip_trace_slot", "polaris_hip_merge_slot", "polaris_hip_build_bvh", "polaris_hip_build_bvh_error",
    "polaris_hip_device_identity", "polaris_hip_can_access_peer", "polaris_hip_peer_info", "polaris_hip_merge_counts",
    "polaris_hip_set_denoise", "polaris_hip_read_aov", "polaris_hip_selftest_builtins", "polaris_hip_denoise_planes",
    "polaris_hip_set_temporal", "polaris_hip_reproject_planes", "polaris_hip_set_variance", "polaris_hip_variance_planes",
    "polaris_hip_set_display", "polaris_hip_read_exposure", "polaris_hip_display_planes", "polaris_hip_set_bloom", "polaris_hip_bloom_planes",
    "polaris_hip_reproject_motion_planes", "polaris_hip_read_instance_plane",
    "polaris_hip_reproject_deform_planes", "polaris_hip_read_hit_plane",
    "polaris_hip_update_instances", "polaris_hip_read_scene_records", "polaris_hip_update_vertices",
    "polaris_hip_update_materials", "polaris_hip_update_texture", "polaris_hip_set_lens", "polaris_hip_set_shutter", "polaris_hip_set_projection",
]

_lib = None


def _torch_first() -> None:
    """The load-order rule of INTEGRATION.md section 4, enforced: this image's torch wheel bundles its own libamdhip64, and a
    process in which libpolaris_hip.so (system libamdhip64) is loaded BEFORE torch has created its GPU context ends up with
    polaris_hip_device_count() == 0.  If torch is already imported, make it touch the GPU now, before the library loads."""
    import sys

    torch = sys.modules.get("torch")
    if torch is None:
        return
    try:
        if torch.cuda.is_available() and not torch.cuda.is_initialized():
            torch.cuda.init()
    except Exception as e:  # a broken torch install must not be reported as a tracer problem later
        raise RuntimeError(f"polaris_amd: torch is imported but its GPU context cannot be created ({e}); "
                           f"libpolaris_hip.so must be loaded after torch has touched the GPU (INTEGRATION.md section 4)") from e


def check_load_order(lib) -> None:
    """Fail loudly on the other half of the trap: the library was loaded first, torch came later and sees GPUs the library
    does not.  Called by HipTracer.Init before it reports 'no device'."""
    import sys

    torch = sys.modules.get("torch")
    if torch is None or lib.polaris_hip_device_count() > 0:
        return
    try:
        seen = torch.cuda.device_count()
    except Exception:
        seen = 0
    if seen > 0:
        raise RuntimeError(f"libpolaris_hip.so sees no HIP device while torch sees {seen}: the library was loaded before torch "
                           f"created its GPU context (this image's torch bundles its own libamdhip64).  Import torch and call "
                           f"torch.cuda.init() before the first polaris_amd.ctypes_api.load_library() / HipTracer() "
                           f"(INTEGRATION.md section 4)")


def load_library(path: str | None = None) -> C.CDLL:
    """Load libpolaris_hip.so (built in-tree by __graft_entry__.build()).  Fails loudly if absent:
    there is no CPU fallback for the product path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("POLARIS_HIP_LIB") or LIB_PATH  # env override: A/B builds while tuning
    if not os.path.exists(p):
        raise RuntimeError(f"{p} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                           f"g.build()'); the tracer has no CPU fallback")
    _torch_first()
    lib = C.CDLL(p)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    lib.polaris_hip_abi_version.restype = i32
    lib.polaris_hip_device_count.restype = i32
    lib.polaris_hip_device_info.argtypes = [i32, C.c_char_p, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64)]
    lib.polaris_hip_create.argtypes = [i32, C.POINTER(vp)]
    lib.polaris_hip_destroy.argtypes = [vp]
    lib.polaris_hip_destroy.restype = None
    lib.polaris_hip_last_error.argtypes = [vp]
    lib.polaris_hip_last_error.restype = C.c_char_p
    lib.polaris_hip_resize.argtypes = [vp, u32, u32]
    lib.polaris_hip_upload_scene.argtypes = [vp, C.POINTER(SceneView)]
    lib.polaris_hip_set_camera.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.polaris_hip_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.polaris_hip_trace.argtypes = [vp, C.POINTER(BlockRequest), C.POINTER(u32), C.c_size_t, C.POINTER(TraceStats)]
    lib.polaris_hip_merge.argtypes = [vp, vp, C.POINTER(BlockRequest)]
    lib.polaris_hip_export_block.argtypes = [vp, C.POINTER(BlockRequest), vp]
    lib.polaris_hip_merge_device.argtypes = [vp, vp, C.POINTER(BlockRequest)]
    lib.polaris_hip_reset_frame.argtypes = [vp]
    lib.polaris_hip_sync_framebuffer.argtypes = [vp, C.POINTER(BlockRequest)]
    lib.polaris_hip_read_framebuffer.argtypes = [vp, vp, C.c_size_t]
    lib.polaris_hip_read_accumulator.argtypes = [vp, i32, vp, C.c_size_t]
    lib.polaris_hip_tap_primary.argtypes = [vp, C.POINTER(BlockRequest), u32, vp, vp, vp, vp]
    lib.polaris_hip_probe.argtypes = [vp, i32, u32, u32, vp, vp]
    lib.polaris_hip_probe_intersect.argtypes = [vp, vp, u32, i32, vp, vp, vp]
    lib.polaris_hip_selftest_rcp.argtypes = [vp, C.c_float, C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(u32)]
    lib.polaris_hip_reset_epoch.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.polaris_hip_wait_reset.argtypes = [vp, C.c_uint64]
    lib.polaris_hip_kernel_symbol.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.polaris_hip_shade_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t]
    lib.polaris_hip_kernel_ms.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.polaris_hip_ipc_export.argtypes = [vp, u32, C.POINTER(IpcExport)]
    lib.polaris_hip_ipc_open.argtypes = [vp, C.POINTER(IpcExport), C.POINTER(vp)]
    lib.polaris_hip_ipc_close.argtypes = [vp, vp]
    lib.polaris_hip_merge_ipc.argtypes = [vp, vp, u32, C.POINTER(BlockRequest)]
    lib.polaris_hip_trace_slot.argtypes = [vp, C.POINTER(u32)]
    lib.polaris_hip_merge_slot.argtypes = [vp, vp, u32, C.POINTER(BlockRequest)]
    lib.polaris_hip_build_bvh.argtypes = [i32, C.POINTER(BvhBuildInput), vp, u32, C.POINTER(u32), vp, vp, C.POINTER(C.c_double)]
    lib.polaris_hip_build_bvh_error.restype = C.c_char_p
    lib.polaris_hip_device_identity.argtypes = [i32, C.POINTER(DeviceIdentity)]
    lib.polaris_hip_can_access_peer.argtypes = [i32, i32, C.POINTER(i32)]
    lib.polaris_hip_peer_info.argtypes = [vp, C.POINTER(PeerInfo)]
    lib.polaris_hip_merge_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.polaris_hip_set_denoise.argtypes = [vp, C.POINTER(DenoiseParams)]
    lib.polaris_hip_read_aov.argtypes = [vp, i32, vp, C.c_size_t]
    lib.polaris_hip_selftest_builtins.argtypes = [vp, u32, C.c_uint64, C.c_uint64, vp, vp]
    lib.polaris_hip_denoise_planes.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, C.c_float, C.c_float, C.POINTER(DenoiseParams), vp, vp]
    lib.polaris_hip_set_lens.argtypes = [vp, C.POINTER(LensParams)]
    lib.polaris_hip_set_shutter.argtypes = [vp, C.POINTER(ShutterParams)]
    lib.polaris_hip_set_projection.argtypes = [vp, C.POINTER(ProjectionParams)]
    lib.polaris_hip_set_temporal.argtypes = [vp, C.POINTER(TemporalParams)]
    lib.polaris_hip_set_variance.argtypes = [vp, C.POINTER(VarianceParams)]
    lib.polaris_hip_set_display.argtypes = [vp, C.POINTER(DisplayParams)]
    lib.polaris_hip_read_exposure.argtypes = [vp, C.POINTER(ExposureInfo), vp]
    lib.polaris_hip_display_planes.argtypes = [vp, vp, u32, u32, u32, u32, C.c_float, C.c_float, C.POINTER(DisplayParams), C.POINTER(C.c_float), vp, vp,
                                               C.POINTER(ExposureInfo)]
    lib.polaris_hip_set_bloom.argtypes = [vp, C.POINTER(BloomParams)]
    lib.polaris_hip_bloom_planes.argtypes = [vp, vp, u32, u32, u32, u32, C.c_float, C.c_float, C.POINTER(DisplayParams), C.POINTER(BloomParams),
                                             C.POINTER(C.c_float), vp, vp, C.POINTER(u32)]
    lib.polaris_hip_variance_planes.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, u32, C.c_float, C.POINTER(DenoiseParams),
                                                C.POINTER(VarianceParams), vp, vp, vp]
    lib.polaris_hip_reproject_planes.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, C.POINTER(TemporalParams), vp]
    lib.polaris_hip_reproject_motion_planes.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp,
                                                        C.POINTER(TemporalParams), vp, vp, vp]
    lib.polaris_hip_read_instance_plane.argtypes = [vp, vp, C.c_size_t]
    lib.polaris_hip_reproject_deform_planes.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp,
                                                        C.POINTER(TemporalParams), vp, vp, vp, vp, vp, vp, u32]
    lib.polaris_hip_read_hit_plane.argtypes = [vp, vp, C.c_size_t]
    lib.polaris_hip_update_instances.argtypes = [vp, C.POINTER(InstanceUpdate)]
    lib.polaris_hip_read_scene_records.argtypes = [vp, i32, vp, C.c_size_t]
    lib.polaris_hip_update_vertices.argtypes = [vp, C.POINTER(VertexUpdate)]
    lib.polaris_hip_update_materials.argtypes = [vp, C.POINTER(MaterialUpdate)]
    lib.polaris_hip_update_texture.argtypes = [vp, u32, vp, C.c_size_t]
    for name in C_ABI_SYMBOLS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int and name not in ("polaris_hip_device_count", "polaris_hip_abi_version"):
            pass
    if path is None:
        _lib = lib
    return lib
