"""The denoiser's filter on the MI355X over the CPU suite's matrix and its edges, through polaris_hip_denoise_planes: the launches
of a denoised sync (polaris_hip.hip launch_steps) on caller planes, so shapes, parameters and planes no scene produces are
reached.

Bars, per (shape, parameters, planes): the DENOISED rows equal the CPU restatement (polaris_host_denoise) bit for bit (NaN equal
to NaN) and lie within the CPU test's rtol 1e-5 / atol 1e-6 of the independent numpy statement (gbuffer_oracle.atrous); the bytes
equal the oracle's tone-map of them with weight 1; rows outside the request come back untouched.  A +inf accumulator damages no
pixel beyond the filter's footprint, 2 (2^K - 1) pixels each way after K iterations."""
import numpy as np
import pytest

import gbuffer_oracle as G
from conftest import make_hip_tracer
from gbuffer_oracle import leaf_word, random_planes
from polaris_amd import ctypes_api as T
from test_denoise_cpu import PARAMS as CPU_PARAMS

pytestmark = pytest.mark.gpu

F = np.float32
WEIGHT, EXPOSURE = F(1.0 / F(7)), F(1.2)

# (W, H, block_y, block_h): the CPU suite's four, a single pixel, one column, one row, rows narrower than a workgroup (a
# workgroup straddles rows), and the last row alone
SHAPES = [(61, 37, 0, None), (300, 9, 0, None), (97, 61, 13, 29), (257, 20, 19, 1), (1, 1, 0, None), (1, 50, 0, None), (50, 1, 0, None),
          (513, 3, 0, None), (61, 37, 36, 1)]
PARAMS = CPU_PARAMS + [
    dict(iterations=1, normal_power_log2=5, sigma_depth=0.1, sigma_luminance=4.0),   # the first iteration is also the last
    dict(iterations=8, normal_power_log2=3, sigma_depth=0.5, sigma_luminance=2.0),   # stride 128: wider than most frames here
    dict(iterations=3, normal_power_log2=5, sigma_depth=1e-6, sigma_luminance=1e-6),
    dict(iterations=3, normal_power_log2=5, sigma_depth=1e6, sigma_luminance=1e6),
]


def _filtered(rng, H, W, a=None):
    guide, albedo = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    guide[..., :3] = (0.0, 0.0, 1.0)
    guide[..., 3] = 2.0
    albedo[..., :3] = rng.random((H, W, 3)) if a is None else a
    albedo[..., 3] = leaf_word(np.full((H, W), T.BXDF_DIFFUSE))
    return guide, albedo


def plane_random(rng, H, W):
    return random_planes(rng, H, W)


def plane_all_miss(rng, H, W):
    acc, guide, albedo = random_planes(rng, H, W)
    guide[...] = (0, 0, 0, G.FLT_MAX)
    albedo[..., :3] = 1.0
    albedo[..., 3] = leaf_word(np.full((H, W), -1))
    return acc, guide, albedo


def plane_all_emitter(rng, H, W):
    acc, guide, albedo = random_planes(rng, H, W)
    albedo[..., 3] = leaf_word(np.full((H, W), T.BXDF_EMISSIVE))
    return acc, guide, albedo


def plane_zero_radiance(rng, H, W):
    acc, guide, albedo = random_planes(rng, H, W)
    acc[...] = 0.0
    return acc, guide, albedo


def plane_dark_albedo(rng, H, W):
    """Albedo channels exactly 0 or exactly the demodulation floor 1e-3."""
    acc, guide, albedo = random_planes(rng, H, W)
    albedo[..., :3] = np.where(rng.random((H, W, 3)) < 0.5, F(0.0), F(1e-3))
    return acc, guide, albedo


def plane_subnormal_weights(rng, H, W):
    """Normals alternating by 0.40 .. 0.45 rad (plus 1e-3 rad of jitter) under P = 10: max(0, n_i . n_j)^1024 of neighbours of
    the other parity lands between 1e-35 and 0, through the subnormals.  Those neighbours carry radiance 1e30 and the centres 0,
    so a device that flushed the subnormal weights would write 0 where the CPU writes ~1e-10."""
    gy, gx = np.mgrid[0:H, 0:W]
    odd = (gx + gy) % 2 == 1
    theta = np.where(odd, 0.40 + 0.05 * rng.random((H, W)), 0.0) + 1e-3 * rng.random((H, W))
    guide, albedo = _filtered(rng, H, W, a=0.5)
    guide[..., 0], guide[..., 1], guide[..., 2] = np.sin(theta), 0.0, np.cos(theta)
    acc = np.zeros((H, W, 4), F)
    acc[..., :3] = np.where(odd, F(0.0), F(1e30))[..., None]
    return acc, guide, albedo


def plane_depth_span(rng, H, W):
    """Hit distances from 1e-4 to 1e4."""
    acc, guide, albedo = random_planes(rng, H, W)
    hit = guide[..., 3] < G.FLT_MAX
    guide[..., 3] = np.where(hit, (10.0 ** rng.uniform(-4, 4, (H, W))).astype(F), G.FLT_MAX)
    return acc, guide, albedo


def plane_inf_pixel(rng, H, W):
    """One filtered pixel whose accumulator is +inf."""
    acc, guide, albedo = random_planes(rng, H, W)
    y, x = H // 2, W // 2
    acc[y, x, 0] = np.inf
    guide[y, x] = (0.0, 0.0, 1.0, 2.0)
    albedo[y, x] = (0.5, 0.5, 0.5, leaf_word([T.BXDF_DIFFUSE])[0])
    return acc, guide, albedo


PLANES = {f.__name__[len("plane_"):]: f for f in (plane_random, plane_all_miss, plane_all_emitter, plane_zero_radiance, plane_dark_albedo,
                                                   plane_subnormal_weights, plane_depth_span, plane_inf_pixel)}


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


@pytest.fixture(scope="module")
def tracer(built):
    from polaris_amd import scenes

    tr = make_hip_tracer(scenes.SCENES["cornell-diffuse"](), 8, 8)
    yield tr
    tr.Close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("plane", list(PLANES))
@pytest.mark.parametrize("pi", range(len(PARAMS)))
@pytest.mark.parametrize("W,H,block_y,block_h", SHAPES)
def test_device_filter_equals_cpu(tracer, host, oracle, W, H, block_y, block_h, pi, plane):
    rng = np.random.default_rng(7919 * pi + 31 * W + H + 5 * block_y)
    acc, guide, albedo = PLANES[plane](rng, H, W)
    p = dict(PARAMS[pi])
    if plane == "subnormal_weights":
        p["normal_power_log2"] = 10
    y1 = H if block_h is None else block_y + block_h
    rows = slice(block_y, y1)
    before = rng.standard_normal((H, W, 4)).astype(F)               # what the rows outside the request must keep
    fb_before = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)

    den, fb = tracer.denoise_planes(acc, guide, albedo, weight=WEIGHT, exposure=EXPOSURE, block_y=block_y, block_h=block_h,
                                    denoised=before, rgba=fb_before, **p)
    want = host.denoise(acc, WEIGHT, guide, albedo, block_y=block_y, block_h=block_h, out=before, **p)

    # outside the request: untouched
    outside = np.ones(H, bool)
    outside[rows] = False
    assert np.array_equal(den[outside].view(np.uint32), before[outside].view(np.uint32))
    assert np.array_equal(fb[outside], fb_before[outside])
    # the CPU restatement, bit for bit (NaN equal to NaN)
    if not same_bits(den, want):
        bad = np.argwhere((den.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(den) & np.isnan(want)))
        y, x, c = bad[0]
        pytest.fail(f"{len(bad)} values differ from polaris_host_denoise; first at (y={y}, x={x}, c={c}): device {den[y, x, c]!r} "
                    f"(0x{den[y, x, c:c + 1].view(np.uint32)[0]:08x}), cpu {want[y, x, c]!r}")
    # the bytes: the oracle's tone-map of the DENOISED rows with weight 1
    assert np.array_equal(fb[rows].reshape(-1, 4), oracle.tonemap(den[rows], 1.0, EXPOSURE)), "frame bytes != oracle tone-map"

    # the independent statement, within the CPU suite's tolerance; a +inf accumulator: damage stays in the footprint
    ref = G.atrous(acc, WEIGHT, guide, albedo, block_y=block_y, block_h=block_h, **p)[rows]
    got = den[rows, :, :3]
    keep = np.ones(got.shape[:2], bool)
    if plane == "inf_pixel":
        reach = 2 * ((1 << p["iterations"]) - 1)
        gy, gx = np.mgrid[block_y:y1, 0:W]
        inside = (np.abs(gy - H // 2) <= reach) & (np.abs(gx - W // 2) <= reach)
        bad = ~np.isfinite(got).all(axis=-1)
        assert not (bad & ~inside).any(), f"non-finite values beyond the {reach}-pixel footprint of the +inf pixel"
        keep = ~inside
    np.testing.assert_allclose(got[keep], ref[keep], rtol=1e-5, atol=1e-6)


def test_denoise_planes_refuses_bad_arguments(tracer):
    from polaris_amd.tracer import TracerError

    acc = np.zeros((4, 5, 4), F)
    guide, albedo = _filtered(np.random.default_rng(0), 4, 5)
    for bad in (dict(iterations=0), dict(iterations=9), dict(normal_power_log2=11), dict(sigma_depth=1e-9), dict(block_y=4, block_h=1),
                dict(block_y=2, block_h=3), dict(block_h=0)):
        with pytest.raises(TracerError):
            tracer.denoise_planes(acc, guide, albedo, weight=1.0, exposure=1.0, **bad)
