"""Temporal reprojection on the CPU (no GPU): polaris_host_reproject / polaris_host_temporal_combine -- the restatements the GPU
kernels are compared with bit for bit (tests/test_gpu_temporal.py) -- against an independent numpy statement of the algorithm
(tests/temporal_oracle.py), engineered moves and rejections, and the quality bars the feature exists for, on oracle traces."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gbuffer_oracle as G
import temporal_oracle as TO
from gbuffer_oracle import FLT_MAX, leaf_word
from polaris_amd import ctypes_api as T

F = np.float32
DEFAULTS = T.TEMPORAL_DEFAULTS


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    return host_api


BOX = [dict(n=(0, 0, 1), d=-2.5, lo=(-0.6, -0.5, -2.5), hi=(0.4, 0.7, -2.5), leaf=T.BXDF_DIFFUSE, albedo=(0.8, 0.2, 0.2)),
       dict(n=(1, 0, 0), d=0.4, lo=(0.4, -0.5, -4.0), hi=(0.4, 0.7, -2.5), leaf=T.BXDF_DIFFUSE, albedo=(0.2, 0.8, 0.2))]
FLOOR = dict(n=(0, 1, 0), d=-1.2, lo=(-50, -1.2, -50), hi=(50, -1.2, 50), leaf=T.BXDF_CONDUCTOR, albedo=(0.9, 0.9, 0.9))
LAMP = dict(n=(0, -1, 0), d=-1.0, lo=(-0.3, 1.0, -3.5), hi=(0.3, 1.0, -3.0), leaf=T.BXDF_EMISSIVE, albedo=(1, 1, 1))
ROOM = [TO.WALL, FLOOR, LAMP] + BOX


def history_planes(rng, H, W, zero_frac=0.05):
    hist = np.zeros((H, W, 4), F)
    hist[..., :3] = (rng.random((H, W, 3)) * 3).astype(F)
    hist[..., 3] = rng.integers(1, 80, (H, W)).astype(F)
    hist[..., 3][rng.random((H, W)) < zero_frac] = 0
    return hist


def both(host, hist, pe, pf, pg, pa, e, f, g, a, **kw):
    got = host.reproject(hist, pg, pa, pe, pf, g, a, e, f, **kw)
    want, margin = TO.reproject(hist, pg, pa, pe, pf, g, a, e, f, **kw)
    return got, want, margin


def random_move(rng):
    look = np.array([0, 0, -1.0]) + 0.08 * rng.standard_normal(3)
    return TO.pinhole(0.15 * rng.standard_normal(3), look=look, fov_deg=40 + 10 * rng.random())


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("W,H", [(64, 48), (37, 53)])
def test_matches_independent_statement(host, seed, W, H):
    rng = np.random.default_rng(seed + 100 * W)
    pe, pf = random_move(rng)
    e, f = random_move(rng)
    pg, pa = TO.trace_planes(pe, pf, W, H, ROOM)
    g, a = TO.trace_planes(e, f, W, H, ROOM)
    # smooth fields (float32 places a projected point within ~1e-4 pixel, so a 1e-5 tolerance needs gentle gradients), with holes
    gy, gx = np.mgrid[0:H, 0:W] / 16.0
    hist = np.zeros((H, W, 4), F)
    hist[..., 0], hist[..., 1], hist[..., 2] = 1 + 0.5 * np.sin(gx), 1 + 0.5 * np.cos(gy), 0.5 + 0.1 * gx * gy
    hist[..., 3] = 24 + 8 * np.sin(gx + gy)
    hist[..., 3][rng.random((H, W)) < 0.05] = 0
    hist[rng.random((H, W)) < 0.01, 0] = np.inf
    pa[..., 3][rng.random((H, W)) < 0.03] = leaf_word(T.BXDF_DIELECTRIC)
    kw = dict(max_history=int(rng.integers(1, 64)), normal_threshold=float(rng.uniform(0.5, 0.99)), depth_threshold=float(rng.uniform(0.02, 0.3)))
    got, want, margin = both(host, hist, pe, pf, pg, pa, e, f, g, a, **kw)
    sure = margin > 1e-4
    assert sure.mean() > 0.8
    np.testing.assert_allclose(got[sure], want[sure], rtol=1e-5, atol=1e-5)
    assert (got[sure, 3] > 0).mean() > 0.3 and (got[sure, 3] == 0).any()
    filt = G.filtered_mask(a)
    assert np.all(got[~filt] == 0)


def test_camera_moved_to_itself_reprojects_every_pixel_onto_itself(host):
    rng = np.random.default_rng(7)
    W, H = 80, 60
    e, f = TO.pinhole((0.1, 0.2, 0.3), look=(0.05, -0.02, -1))
    g, a = TO.trace_planes(e, f, W, H, ROOM)
    hist = history_planes(rng, H, W, zero_frac=0)
    got = host.reproject(hist, g, a, e, f, g, a, e, f, **DEFAULTS)
    filt = G.filtered_mask(a)
    # (float32 lands each point within ~1e-4 pixel of its own centre: the neighbours' weights are that small)
    np.testing.assert_allclose(got[filt, :3], hist[filt, :3], atol=2e-3)
    np.testing.assert_allclose(got[filt, 3], np.minimum(hist[filt, 3], DEFAULTS["max_history"]), atol=2e-2)
    assert np.all(got[~filt] == 0)


@pytest.mark.parametrize("k", [1, 3])
def test_sideways_eye_shift_over_a_fronto_parallel_plane_shifts_the_history(host, k):
    W, H = 64, 64
    D, fov = 4.0, 45.0
    pixel = 2 * D * np.tan(np.radians(fov / 2)) / W        # width of a pixel on the wall
    pe, pf = TO.pinhole((0, 0, 0), fov_deg=fov)
    e, f = TO.pinhole((k * pixel, 0, 0), fov_deg=fov)     # (the corners are eye-relative: a translation keeps them)
    assert np.array_equal(pf, f)
    pg, pa = TO.trace_planes(pe, pf, W, H, [TO.WALL])
    g, a = TO.trace_planes(e, f, W, H, [TO.WALL])
    hist = np.zeros((H, W, 4), F)
    gy, gx = np.mgrid[0:H, 0:W]
    hist[..., 0] = gx
    hist[..., 1] = gy
    hist[..., 2] = 1.0
    hist[..., 3] = 8
    got = host.reproject(hist, pg, pa, pe, pf, g, a, e, f, **DEFAULTS)
    inner = slice(0, W - k - 1)
    np.testing.assert_allclose(got[:, inner, 0], gx[:, inner] + k, atol=2e-3)
    np.testing.assert_allclose(got[:, inner, 1], gy[:, inner], atol=2e-3)
    assert np.all(got[:, inner, 3] == 8)
    assert np.all(got[:, W - k + 1:, 3] == 0)                 # (projected out of the old frame)


# ---- rejections: each must give m = 0, and TEMPORAL = acc * weight bit for bit there -------------------------------------
def check_rejected(host, prior, mask, rng):
    assert mask.any()
    assert np.all(prior[mask] == 0), f"{int((prior[mask, 3] != 0).sum())} pixels kept history"
    H, W = prior.shape[:2]
    acc = np.zeros((H, W, 4), F)
    acc[..., :3] = (rng.random((H, W, 3)) * 20).astype(F)
    for accumulated, spp in ((0, 1), (6, 3)):
        tmp = host.temporal_combine(acc, prior, accumulated, spp)
        weight = F(1.0 / F(accumulated + spp))
        assert np.array_equal(tmp[mask, :3].view(np.uint32), (acc[mask, :3] * weight).view(np.uint32))
        assert np.all(tmp[mask, 3] == accumulated + spp)


def room_pair(W=64, H=64, dx=0.25):
    pe, pf = TO.pinhole((0, 0, 0))
    e, f = TO.pinhole((dx, 0, 0))
    pg, pa = TO.trace_planes(pe, pf, W, H, ROOM)
    g, a = TO.trace_planes(e, f, W, H, ROOM)
    return pe, pf, pg, pa, e, f, g, a


def test_reject_disocclusion_behind_a_box(host):
    rng = np.random.default_rng(1)
    pe, pf, pg, pa, e, f, g, a = room_pair()
    hist = history_planes(rng, *g.shape[:2], zero_frac=0)
    got, want, margin = both(host, hist, pe, pf, pg, pa, e, f, g, a, **DEFAULTS)
    # wall pixels of the new view whose point the box hid from the old one: every tap is a box face (another depth)
    wall = np.isclose(g[..., 2], 1) & (np.abs(g[..., 3] - 4 / np.abs(TO.centre_dirs(e, f, 64, 64)[..., 2])) < 1e-3)
    disoccluded = wall & (want[..., 3] == 0) & np.isfinite(margin)
    assert disoccluded.sum() >= 20
    check_rejected(host, got, disoccluded, rng)
    assert (got[wall & ~disoccluded, 3] > 0).mean() > 0.9


def test_reject_leaf_change(host):
    rng = np.random.default_rng(2)
    pe, pf, pg, pa, e, f, g, a = room_pair(dx=0.05)
    filt = G.filtered_mask(a)
    pa2 = pa.copy()
    pa2[..., 3] = leaf_word(T.BXDF_ROUGH_CONDUCTOR)
    hist = history_planes(rng, *g.shape[:2], zero_frac=0)
    assert (host.reproject(hist, pg, pa, pe, pf, g, a, e, f, **DEFAULTS)[filt, 3] > 0).mean() > 0.9
    check_rejected(host, host.reproject(hist, pg, pa2, pe, pf, g, a, e, f, **DEFAULTS), filt, rng)


def test_reject_normal_flip(host):
    rng = np.random.default_rng(3)
    pe, pf, pg, pa, e, f, g, a = room_pair(dx=0.05)
    pg2 = pg.copy()
    pg2[..., :3] *= -1
    hist = history_planes(rng, *g.shape[:2], zero_frac=0)
    check_rejected(host, host.reproject(hist, pg2, pa, pe, pf, g, a, e, f, **DEFAULTS), G.filtered_mask(a), rng)


def test_reject_depth_jump(host):
    rng = np.random.default_rng(4)
    pe, pf, pg, pa, e, f, g, a = room_pair(dx=0.05)
    pg2 = pg.copy()
    pg2[..., 3] *= F(1.25)
    hist = history_planes(rng, *g.shape[:2], zero_frac=0)
    check_rejected(host, host.reproject(hist, pg2, pa, pe, pf, g, a, e, f, **DEFAULTS), G.filtered_mask(a), rng)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_reject_non_finite_history(host, bad):
    rng = np.random.default_rng(5)
    W = H = 48
    e, f = TO.pinhole((0, 0, 0))
    g, a = TO.trace_planes(e, f, W, H, [TO.WALL])
    hist = history_planes(rng, H, W, zero_frac=0)
    hist[20:24, 10:14, 1] = bad                       # a 4 x 4 block: the inner 2 x 2 see only non-finite taps
    got = host.reproject(hist, g, a, e, f, g, a, e, f, **DEFAULTS)
    mask = np.zeros((H, W), bool)
    mask[21:23, 11:13] = True
    check_rejected(host, got, mask, rng)
    assert np.all(np.isfinite(got))
    assert np.all(got[:18, :, 3] > 0)


def test_reject_point_behind_the_old_camera(host):
    rng = np.random.default_rng(6)
    W = H = 48
    pe, pf = TO.pinhole((0, 0, -6), look=(0, 0, -1))          # the wall (z = -4) lies behind it
    e, f = TO.pinhole((0, 0, 0))
    g, a = TO.trace_planes(e, f, W, H, [TO.WALL])
    hist = history_planes(rng, H, W, zero_frac=0)
    check_rejected(host, host.reproject(hist, g, a, pe, pf, g, a, e, f, **DEFAULTS), G.filtered_mask(a), rng)
    # in front of the wall, the same camera does see it
    pe2, pf2 = TO.pinhole((0, 0, -1), look=(0, 0, -1))
    pg2, pa2 = TO.trace_planes(pe2, pf2, W, H, [TO.WALL])
    assert (host.reproject(hist, pg2, pa2, pe2, pf2, g, a, e, f, **DEFAULTS)[..., 3] > 0).mean() > 0.5


@pytest.mark.parametrize("corner,delta", [(3, (0.01, 0, 0, 0)), (0, (0, 0, 0, 0.5)), (2, (0, 0, 0, -1e-6))])
def test_reject_non_parallelogram_corners(host, corner, delta):
    rng = np.random.default_rng(8)
    W = H = 40
    e, f = TO.pinhole((0, 0, 0))
    g, a = TO.trace_planes(e, f, W, H, [TO.WALL])
    hist = history_planes(rng, H, W, zero_frac=0)
    assert (host.reproject(hist, g, a, e, f, g, a, e, f, **DEFAULTS)[..., 3] > 0).all()
    f2 = f.copy()
    f2[corner] += np.asarray(delta, F)
    check_rejected(host, host.reproject(hist, g, a, e, f2, g, a, e, f, **DEFAULTS), np.ones((H, W), bool), rng)
    f3 = f.copy()
    f3[3, 0] += F(1e-4)                                   # a skew under 1e-3 |tr - tl| is still a parallelogram
    assert (host.reproject(hist, g, a, e, f3, g, a, e, f, **DEFAULTS)[..., 3] > 0).mean() > 0.95


def test_misses_and_emitters_get_no_history(host):
    rng = np.random.default_rng(9)
    W = H = 64
    pe, pf = TO.pinhole((0, 0, 0))
    e, f = TO.pinhole((0.02, 0, 0))
    room = [LAMP] + BOX                                   # (no wall: misses behind the box)
    pg, pa = TO.trace_planes(pe, pf, W, H, room)
    g, a = TO.trace_planes(e, f, W, H, room)
    leaf = np.ascontiguousarray(a[..., 3]).view(np.uint32)
    hist = history_planes(rng, H, W, zero_frac=0)
    hist[..., 3] = 5                                      # (the history of misses and emitters has counts too)
    got = host.reproject(hist, pg, pa, pe, pf, g, a, e, f, **DEFAULTS)
    for m in (leaf == 0xFFFFFFFF, leaf == T.BXDF_EMISSIVE):
        check_rejected(host, got, m, rng)
    assert (got[G.filtered_mask(a), 3] > 0).mean() > 0.9


def test_combine_blends_where_history_exists(host):
    rng = np.random.default_rng(10)
    H, W = 9, 13
    acc = (rng.random((H, W, 4)) * 10).astype(F)
    prior = (rng.random((H, W, 4)) * 2).astype(F)
    prior[..., 3] = rng.integers(0, 20, (H, W)).astype(F)
    got = host.temporal_combine(acc, prior, 5, 2)
    want = TO.combine(acc, prior, 5, 2)
    np.testing.assert_allclose(got, want, rtol=1e-6)
    before = np.full((H, W, 4), 7, F)
    part = host.temporal_combine(acc, prior, 5, 2, block_y=3, block_h=4, out=before)
    assert np.array_equal(part[3:7], got[3:7]) and np.all(part[:3] == 7) and np.all(part[7:] == 7)


@pytest.mark.parametrize("bad", [dict(max_history=4097), dict(normal_threshold=1.5), dict(normal_threshold=float("nan")),
                                 dict(depth_threshold=-0.1), dict(depth_threshold=float("inf")), dict(depth_threshold=2e6),
                                 dict(normal_threshold=-1.01)])
def test_malformed_params_are_rejected(host, bad):
    W = H = 4
    e, f = TO.pinhole((0, 0, 0))
    g, a = TO.trace_planes(e, f, W, H, [TO.WALL])
    kw = dict(DEFAULTS)
    kw.update(bad)
    with pytest.raises(ValueError):
        host.reproject(np.zeros_like(g), g, a, e, f, g, a, e, f, **kw)


def test_malformed_struct_and_rows_are_rejected(host):
    lib = host.load()
    W = H = 4
    e, f = TO.pinhole((0, 0, 0))
    g, a = TO.trace_planes(e, f, W, H, [TO.WALL])
    out = np.zeros_like(g)
    p = T.temporal_params(**DEFAULTS)
    args = lambda pp, w=W: (g.ctypes.data, g.ctypes.data, a.ctypes.data, e.ctypes.data, f.ctypes.data, g.ctypes.data, a.ctypes.data,  # noqa: E731
                            e.ctypes.data, f.ctypes.data, w, H, C.byref(pp), out.ctypes.data)
    assert lib.polaris_host_reproject(*args(p)) == 0
    assert lib.polaris_host_reproject(*args(p, 0)) == 2
    p.struct_size = 12
    assert lib.polaris_host_reproject(*args(p)) == 2
    assert lib.polaris_host_temporal_combine(g.ctypes.data, g.ctypes.data, 0, 1, W, H, 2, 3, out.ctypes.data) == 2
    assert lib.polaris_host_temporal_combine(g.ctypes.data, g.ctypes.data, 0, 0, W, H, 0, 1, out.ctypes.data) == 2


def test_camera_move_restates_the_reference_camera(host):
    sc = host.read_scene(content="camera_eye 0 1 5\ncamera_look 0 1 0\ncamera_fov 50\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", name="tri")
    e0, f0 = host.camera_move(sc.camera, [])
    assert np.array_equal(e0, sc.eye) and np.array_equal(f0, sc.frustum)
    e1, f1 = host.camera_move(sc.camera, [("right", 0.5)])
    np.testing.assert_allclose(e1, sc.eye + np.array([0.5, 0, 0], F), atol=1e-6)
    np.testing.assert_allclose(f1, f0, atol=1e-6)           # (a translation keeps the eye-relative corners)
    e2, _ = host.camera_move(sc.camera, [("right", 0.5), ("forward", 1.0), ("up", 0.25)])
    np.testing.assert_allclose(e2, sc.eye + np.array([0.5, 0.25, -1.0], F), atol=1e-5)
    with pytest.raises(KeyError):
        host.camera_move(sc.camera, [("sideways", 1.0)])


# ---- quality: the bars the feature exists for, on oracle traces ----------------------------------------------------------
def moved(sc, dx):
    return dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([dx, 0, 0], F)).astype(F))


def quality_run(host, oracle, sc, N, dx, hist_spp, spp, steps, ref_spp=1024, params=None):
    """RMSE (temporal + a-trous, a-trous alone, the reused fraction, TEMPORAL unfiltered, the mean unfiltered) at the last of `steps` moves by dx, every view traced at spp, the first history
    at hist_spp, both against ref_spp at the last view."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    params = dict(DEFAULTS if params is None else params)
    cam = sc
    acc0, _, _ = oracle.trace(cam, ob.make_request(N, N, spp=hist_spp, bounces=5), scenes.make_seeds(hist_spp, 5, base=7))
    g0, a0, _ = G.gbuffer(oracle, cam, N, N)
    hist = host.temporal_combine(acc0, np.zeros_like(acc0), 0, hist_spp)
    for k in range(1, steps + 1):
        cam_k = moved(sc, dx * k)
        acc, _, _ = oracle.trace(cam_k, ob.make_request(N, N, spp=spp, bounces=5), scenes.make_seeds(spp, 5, base=100 + k))
        g, a, _ = G.gbuffer(oracle, cam_k, N, N)
        prior = host.reproject(hist, g0, a0, cam.eye, cam.frustum, g, a, cam_k.eye, cam_k.frustum, **params)
        hist = host.temporal_combine(acc, prior, 0, spp)
        cam, g0, a0 = cam_k, g, a
    ref, _, _ = oracle.trace(cam, ob.make_request(N, N, spp=ref_spp, bounces=5), scenes.make_seeds(ref_spp, 5, base=99))
    want = ref[..., :3] / ref_spp
    tmp = host.denoise(hist, F(1), g0, a0, **T.DENOISE_DEFAULTS)[..., :3]
    spatial = host.denoise(acc, F(1.0 / F(spp)), g0, a0, **T.DENOISE_DEFAULTS)[..., :3]
    # over the filtered pixels of the last view: misses and emitters pass through both pipelines as the same acc * weight
    filt = G.filtered_mask(a0)
    rmse = lambda x: float(np.sqrt(np.mean((x[filt] - want[filt]) ** 2)))  # noqa: E731
    return rmse(tmp), rmse(spatial), float((prior[filt, 3] > 0).mean()), rmse(hist[..., :3]), rmse(acc[..., :3] / spp)


# Bars from the recorded table (profiles/temporal_quality.txt).  The a-trous filter has an error floor of its own
# at 128^2 (0.074 on cornell-diffuse even at 64 spp), so where the filter alone is already at that floor (cornell-diffuse) temporal
# + a-trous can only match it: the 0.75 bar holds where noise dominates (cornell, one move), and the unfiltered TEMPORAL plane must
# beat the unfiltered 1 spp frame by 4x everywhere.
BAR1 = {"cornell": 0.75, "cornell-diffuse": 1.0}


@pytest.mark.parametrize("name", ["cornell-diffuse", "cornell"])
def test_quality_one_move_at_1_spp(host, oracle, name):
    from polaris_amd import scenes

    t, s, reused, tr, r = quality_run(host, oracle, scenes.SCENES[name](), 128, 0.03, 64, 1, 1)
    print(f"{name}: one move, 1 spp: temporal {t:.4f} spatial {s:.4f} ratio {t / s:.3f} reused {reused:.3f}; unfiltered {tr / r:.3f}")
    assert reused > 0.95
    assert t <= BAR1[name] * s, (t, s)
    assert tr <= 0.25 * r, (tr, r)


@pytest.mark.parametrize("name", ["cornell-diffuse", "cornell"])
def test_quality_chain_of_8_moves_at_1_spp(host, oracle, name):
    from polaris_amd import scenes

    t, s, reused, tr, r = quality_run(host, oracle, scenes.SCENES[name](), 128, 0.01, 64, 1, 8)
    print(f"{name}: 8 moves, 1 spp: temporal {t:.4f} spatial {s:.4f} ratio {t / s:.3f} reused {reused:.3f}; unfiltered {tr / r:.3f}")
    assert t <= 1.0 * s, (t, s)
    assert tr <= 0.3 * r, (tr, r)


@pytest.mark.parametrize("name", ["cornell-diffuse", "cornell"])
def test_quality_prior_does_not_hurt_a_good_frame(host, oracle, name):
    from polaris_amd import scenes

    t, s, _, tr, r = quality_run(host, oracle, scenes.SCENES[name](), 128, 0.03, 64, 64, 1)
    print(f"{name}: one move, 64 spp: temporal {t:.4f} spatial {s:.4f} ratio {t / s:.3f}; unfiltered {tr / r:.3f}")
    assert t <= 1.05 * s, (t, s)
    assert tr <= 1.0 * r, (tr, r)
