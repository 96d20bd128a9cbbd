"""The denoiser's filter on the CPU (no GPU): polaris_host_denoise -- the restatement the GPU kernel is compared with bit for bit
(tests/test_gpu_denoise.py) -- against an independent numpy statement of the algorithm, its properties, and the quality bar the
feature exists for, on G-buffers and traces of the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_oracle as G
from gbuffer_oracle import leaf_word, random_planes
from polaris_amd import ctypes_api as T

F = np.float32
PARAMS = [dict(iterations=4, normal_power_log2=5, sigma_depth=0.1, sigma_luminance=4.0),
          dict(iterations=5, normal_power_log2=7, sigma_depth=0.1, sigma_luminance=1.0),
          dict(iterations=2, normal_power_log2=0, sigma_depth=0.0, sigma_luminance=0.0),
          dict(iterations=8, normal_power_log2=10, sigma_depth=2.0, sigma_luminance=0.5)]


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    return host_api


@pytest.mark.parametrize("W,H,block_y,block_h", [(61, 37, 0, None), (300, 9, 0, None), (97, 61, 13, 29), (257, 20, 19, 1)])
@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_matches_independent_restatement(host, W, H, block_y, block_h, pi):
    rng = np.random.default_rng(1000 * pi + W + H)
    acc, guide, albedo = random_planes(rng, H, W)
    weight = F(1.0 / F(7))
    got = host.denoise(acc, weight, guide, albedo, block_y=block_y, block_h=block_h, **PARAMS[pi])
    want = G.atrous(acc, weight, guide, albedo, block_y=block_y, block_h=block_h, **PARAMS[pi])
    rows = slice(block_y, H if block_h is None else block_y + block_h)
    np.testing.assert_allclose(got[rows, :, :3], want[rows], rtol=1e-5, atol=1e-6)
    filt = G.filtered_mask(albedo[rows])
    assert filt.any() and (~filt).any()


def test_misses_and_emitters_pass_through_bit_equal(host):
    rng = np.random.default_rng(5)
    H, W = 23, 41
    acc, guide, albedo = random_planes(rng, H, W)
    leaves = np.where(rng.random((H, W)) < 0.5, -1, T.BXDF_EMISSIVE).astype(np.int32)
    albedo[..., 3] = leaf_word(leaves)
    weight = F(1.0 / F(3))
    got = host.denoise(acc, weight, guide, albedo)
    assert np.array_equal(got[..., :3].view(np.uint32), (acc[..., :3] * weight).view(np.uint32))


def plane(H, W, normal=(0.0, 0.0, 1.0), t=2.0, leaf=T.BXDF_DIFFUSE, a=(0.5, 0.4, 0.3)):
    guide = np.zeros((H, W, 4), F)
    guide[..., :3] = normal
    guide[..., 3] = t
    albedo = np.zeros((H, W, 4), F)
    albedo[..., :3] = a
    albedo[..., 3] = leaf_word(np.full((H, W), leaf))
    return guide, albedo


@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_constant_field_on_a_plane_is_preserved(host, pi):
    H, W = 40, 70
    guide, albedo = plane(H, W)
    acc = np.zeros((H, W, 4), F)
    acc[..., :3] = (0.7, 1.9, 0.05)
    got = host.denoise(acc, F(0.5), guide, albedo, **PARAMS[pi])
    np.testing.assert_allclose(got[..., :3], np.broadcast_to(acc[..., :3] * F(0.5), got[..., :3].shape), rtol=1e-6, atol=0)


@pytest.mark.parametrize("pi", [0, 1, 3])   # (every one with a normal term: P >= 0 and orthogonal normals weigh 0)
def test_edge_between_orthogonal_half_planes_keeps_its_step(host, pi):
    H, W = 33, 64
    guide, albedo = plane(H, W)
    guide[:, W // 2:, :3] = (1.0, 0.0, 0.0)
    acc = np.zeros((H, W, 4), F)
    acc[:, :W // 2, :3] = (2.0, 0.1, 0.3)
    acc[:, W // 2:, :3] = (0.05, 0.9, 5.0)
    got = host.denoise(acc, F(1), guide, albedo, **PARAMS[pi])
    np.testing.assert_allclose(got[..., :3], acc[..., :3], rtol=1e-6, atol=0)


def test_rows_outside_the_request_are_untouched(host):
    rng = np.random.default_rng(9)
    H, W = 30, 50
    acc, guide, albedo = random_planes(rng, H, W)
    before = rng.random((H, W, 4)).astype(F)
    got = host.denoise(acc, F(0.25), guide, albedo, block_y=11, block_h=7, out=before)
    assert np.array_equal(got[:11], before[:11]) and np.array_equal(got[18:], before[18:])
    assert not np.array_equal(got[11:18], before[11:18])


@pytest.mark.parametrize("bad", [dict(iterations=9), dict(normal_power_log2=11), dict(sigma_depth=-0.1), dict(sigma_luminance=float("nan")),
                                 dict(sigma_depth=float("inf")), dict(sigma_luminance=1e-9), dict(sigma_depth=1e7)])
def test_malformed_params_are_rejected(host, bad):
    H, W = 4, 5
    acc = np.zeros((H, W, 4), F)
    guide, albedo = plane(H, W)
    with pytest.raises(ValueError):
        host.denoise(acc, F(1), guide, albedo, **bad)


def test_malformed_struct_and_rows_are_rejected(host):
    lib = host.load()
    H, W = 4, 5
    acc = np.zeros((H, W, 4), F)
    guide, albedo = plane(H, W)
    out = np.zeros_like(acc)
    p = T.denoise_params()
    args = lambda y, h, pp: (acc.ctypes.data, 1.0, guide.ctypes.data, albedo.ctypes.data, W, H, y, h, C.byref(pp), out.ctypes.data)  # noqa: E731
    assert lib.polaris_host_denoise(*args(0, H, p)) == 0
    assert lib.polaris_host_denoise(*args(2, 3, p)) == 2 and lib.polaris_host_denoise(*args(0, 0, p)) == 2
    p.struct_size = 16
    assert lib.polaris_host_denoise(*args(0, H, p)) == 2


def test_iterations_zero_is_the_running_mean(host):
    rng = np.random.default_rng(3)
    acc, guide, albedo = random_planes(rng, 12, 17)
    got = host.denoise(acc, F(0.125), guide, albedo, iterations=0)
    assert np.array_equal(got[..., :3], acc[..., :3] * F(0.125))


# ---- quality: the bar the feature exists for ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell-diffuse", "cornell"])
def test_quality_at_4_spp_against_1024_spp(host, oracle, name):
    from oracle import pybind as ob
    from polaris_amd import scenes

    N = 128
    sc = scenes.SCENES[name]()
    guide, albedo, _ = G.gbuffer(oracle, sc, N, N)
    noisy, _, _ = oracle.trace(sc, ob.make_request(N, N, spp=4, bounces=5), scenes.make_seeds(4, 5, base=11))
    ref, _, _ = oracle.trace(sc, ob.make_request(N, N, spp=1024, bounces=5), scenes.make_seeds(1024, 5, base=99))
    want = ref[..., :3] / 1024
    den = host.denoise(noisy, F(0.25), guide, albedo, **T.DENOISE_DEFAULTS)[..., :3]
    rmse = lambda x, m=slice(None): float(np.sqrt(np.mean((x[m] - want[m]) ** 2)))  # noqa: E731
    edges = G.edge_mask(guide)
    assert 0.05 < edges.mean() < 0.5
    ratio, edge_ratio = rmse(den) / rmse(noisy[..., :3] / 4), rmse(den, edges) / rmse(noisy[..., :3] / 4, edges)
    assert ratio <= 0.6, ratio
    assert edge_ratio <= 1.0, edge_ratio
