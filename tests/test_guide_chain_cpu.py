"""The option "guide_specular"  on the CPU: the restatement tests/guide_chain_oracle.py against the first-hit
restatement, against planar-mirror geometry worked out independently in float64, through the numpy reprojection of
tests/temporal_oracle.py, and through the CPU filter on oracle traces.  The GPU side is tests/test_gpu_guide_chain.py."""
import functools
import math

import numpy as np
import pytest

import gbuffer_oracle as G
import guide_chain_oracle as GC
import temporal_oracle as TO
from conftest import bits
from polaris_amd import ctypes_api as T

F = np.float32
W, H = 97, 61
SHIFT = 0.02                     # the sideways camera translation of the reprojection experiment, in room widths (the room is 1 wide)
# The reprojection experiment looks at little but the mirror (this field of view) at a resolution where one pixel
# footprint at the unfolded distance, T * 2 tan(fov / 2) / H = 0.0051 T, is well below what "paint on the mirror" gets wrong: the
# eye moves by 0.02, so the point seen at one spot of the mirror moves by 0.02 * L / 0.935 on a surface L past the mirror
# (0.012 on the box, T = 1.5; 0.021 on the wall behind the camera, T = 1.93; more on the floor, which the rays graze).
RW = RH = 121
RFOV = 0.6


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


@functools.lru_cache(maxsize=None)
def room(aspect, dx=0.0, fov=None):
    from polaris_amd import scenes

    kw = {} if fov is None else {"fov": fov}
    return scenes.mirror_room(aspect, eye=(0.5 + dx, 0.5, 0.06), **kw)


_cache = {}


def chained(oracle, sc, w, h, links):
    """The restatement, computed once per (scene, size, links) and shared (nobody writes to it)."""
    key = (id(sc), w, h, links)
    if key not in _cache:
        _cache[key] = (sc, GC.chained_gbuffer(oracle, sc, w, h, links))
    return _cache[key][1]


# ---- 1. N = 0 is the first-hit G-buffer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mirror_room", "cornell"])
def test_no_links_is_the_first_hit_gbuffer(oracle, name):
    from polaris_amd import scenes

    sc = room(W / H) if name == "mirror_room" else scenes.cornell_box("layered", W / H)
    guide, albedo, inst, info = chained(oracle, sc, W, H, 0)
    want_g, want_a, want_info = G.gbuffer(oracle, sc, W, H)
    assert np.array_equal(bits(guide), bits(want_g)) and np.array_equal(bits(albedo), bits(want_a))
    assert np.array_equal(info["textured"], want_info["textured"])
    hit = want_g[..., 3] < G.FLT_MAX
    assert np.array_equal(inst == GC.NO_INSTANCE, ~hit) and np.all(inst[hit] == 0)
    assert np.all(info["k"][hit] == 0) and np.all(info["k"][~hit] == -1)


# ---- 2. chain lengths on mirror_room --------------------------------------------------------------------------------------------
def slab_first_hits(sc, info):
    """Pixels whose first hit is the slab's large face towards the room (x = 0.93)."""
    x = np.asarray(sc.vertices, F)[:, 0].reshape(-1, 3)
    face = np.nonzero(np.all(x == F(0.93), axis=1))[0]
    assert len(face) == 2
    return np.isin(info["first_tri"], face)


def test_chain_lengths(oracle):
    sc = room(W / H)
    guide, albedo, inst, info = chained(oracle, sc, W, H, 4)
    k, typ = info["k"], GC.leaf_types(albedo)
    assert sc.num_triangles <= 400 and len(sc.mesh_instances) == 1
    planar = GC.through_planar_mirror(sc, info)
    assert planar.sum() > 400
    first_conductor = info["first_type"] == T.BXDF_CONDUCTOR
    sphere = first_conductor & ~np.isin(info["first_tri"], GC.planar_mirror_tris(sc))
    assert (sphere & (k == 1)).sum() > 100                        # the mirror sphere, one link
    slab = slab_first_hits(sc, info)
    assert slab.sum() > 300 and np.all(info["first_type"][slab] == T.BXDF_DIELECTRIC)
    assert (slab & (k == 2)).sum() > 0.8 * slab.sum()             # in through one interface, out through the other
    assert np.all(typ[slab & (k == 2)] == T.BXDF_DIFFUSE)
    seen = planar & (typ == T.BXDF_DIFFUSE)
    assert (planar & (typ == T.BXDF_EMISSIVE)).sum() >= 6         # the ceiling light, in the mirror only
    assert not (typ[k == 0] == T.BXDF_EMISSIVE).any()
    assert info["textured"][seen].any() and (seen & ~info["textured"]).any()   # the checker floor and plain surfaces in the mirror
    assert np.all(inst[k >= 1] == GC.NO_INSTANCE) and np.all(inst[k == 0] == 0)
    assert np.all(albedo[planar & (typ == T.BXDF_EMISSIVE)][:, :3] == np.array([0.9, 0.9, 0.95], F))   # A = the mirror's, a = 1
    # N = 1: the slab's pixels stop on its back interface
    _, albedo1, _, info1 = chained(oracle, sc, W, H, 1)
    assert np.all(info1["k"][slab] == 1) and np.all(GC.leaf_types(albedo1)[slab] == T.BXDF_DIELECTRIC)
    assert np.all(info1["k"] <= 1) and k.max() == 4


# ---- 3. planar-mirror geometry, independent of the loop -----------------------------------------------------------------------------
def test_planar_mirror_unfolds_to_the_mirror_image(oracle):
    from polaris_amd import scenes

    sc = room(W / H)
    guide, albedo, _, info = chained(oracle, sc, W, H, 4)
    m = GC.through_planar_mirror(sc, info)
    mz = float(F(scenes.MIRROR_ROOM_MIRROR[2]))
    eye = np.asarray(sc.eye, np.float64)
    eye_m = eye * [1, 1, -1] + [0, 0, 2 * mz]                      # the eye mirrored in the plane z = mz
    p = info["point"][m].astype(np.float64)
    t = guide[m][:, 3].astype(np.float64)
    want_t = np.linalg.norm(p - eye_m, axis=-1)
    print("T: max relative error", np.max(np.abs(t - want_t) / want_t))
    assert np.all(np.abs(t - want_t) <= 1e-5 * want_t)
    d = G.centre_rays(sc, W, H)[:, 4:7].reshape(H, W, 3)[m].astype(np.float64)
    image = p * [1, 1, -1] + [0, 0, 2 * mz]                        # the mirror image of the final hit point
    err = np.linalg.norm(eye + t[:, None] * d - image, axis=-1)
    print("eye + T d: max error / T", np.max(err / t))
    assert np.all(err <= 1e-5 * t)


# ---- 4. reprojection through the planar mirror --------------------------------------------------------------------------------------
def reprojection_experiment(oracle, links):
    """The guides with `links`; the history's colour and every pixel's own position from the followed chains (N = 2).
    Returns (eligible, m, error, bound): the last three over the eligible pixels."""
    a, b = room(RW / RH, 0.0, RFOV), room(RW / RH, SHIFT, RFOV)
    ga, aa, _, ia = chained(oracle, a, RW, RH, 2)
    gb, ab, _, ib = chained(oracle, b, RW, RH, 2)
    elig = GC.reprojection_eligible(b, gb, ab, ib)
    history = np.zeros((RH, RW, 4), F)
    history[..., :3] = ia["point"]
    history[..., 3] = 8
    if links != 2:
        ga, aa, _, _ = chained(oracle, a, RW, RH, links)
        gb_l, ab_l, _, _ = chained(oracle, b, RW, RH, links)
    else:
        gb_l, ab_l = gb, ab
    prior, _ = TO.reproject(history, ga, aa, a.eye, a.frustum, gb_l, ab_l, b.eye, b.frustum)
    err = np.linalg.norm(prior[..., :3] - ib["point"].astype(np.float64), axis=-1)
    bound = gb[..., 3].astype(np.float64) * 2 * math.tan(RFOV / 2) / RH
    return elig, prior[..., 3][elig], err[elig], bound[elig]


def test_reprojection_through_the_planar_mirror(oracle):
    elig, m, err, bound = reprojection_experiment(oracle, 2)
    assert elig.sum() > 0.5 * RW * RH                              # the mirror fills most of the frame
    print("eligible", int(elig.sum()), "with history", float((m > 0).mean()), "max error / bound", float(np.max(err[m > 0] / bound[m > 0])))
    assert (m > 0).mean() >= 0.9
    assert np.all(err[m > 0] <= bound[m > 0])


def test_first_hit_guides_reproject_the_mirror_as_paint(oracle):
    """The same experiment with the N = 0 guides fails its bound on most pixels: the test above can fail."""
    elig, m, err, bound = reprojection_experiment(oracle, 0)
    print("first-hit guides: with history", float((m > 0).mean()), "beyond the bound", float((err > bound).mean()))
    assert (err > bound).mean() > 0.5


# ---- 5. filter quality --------------------------------------------------------------------------------------------------------------
def test_filter_quality_inside_mirrors_and_glass(host, oracle):
    """RMSE of linear radiance at 4 spp against 1024 spp over the pixels seen through a chain whose final leaf is filtered: the
    chained guide (N = 4) may not be worse than the first-hit guide (N = 0) -- the parent's behaviour, no further margin."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    N = 128
    sc = room(1.0)
    g0, a0, _, _ = chained(oracle, sc, N, N, 0)
    g4, a4, _, i4 = chained(oracle, sc, N, N, 4)
    noisy, _, _ = oracle.trace(sc, ob.make_request(N, N, spp=4, bounces=5), scenes.make_seeds(4, 5, base=11))
    ref, _, _ = oracle.trace(sc, ob.make_request(N, N, spp=1024, bounces=5), scenes.make_seeds(1024, 5, base=99))
    want = ref[..., :3] / 1024
    mask = (i4["k"] >= 1) & G.filtered_mask(a4)
    assert mask.sum() > 1500
    rmse = lambda x: float(np.sqrt(np.mean((x[mask] - want[mask]) ** 2)))  # noqa: E731
    base = rmse(noisy[..., :3] / 4)
    r0 = rmse(host.denoise(noisy, F(0.25), g0, a0, **T.DENOISE_DEFAULTS)[..., :3]) / base
    r4 = rmse(host.denoise(noisy, F(0.25), g4, a4, **T.DENOISE_DEFAULTS)[..., :3]) / base
    print(f"denoised / noisy RMSE over {int(mask.sum())} chain pixels: N = 0 {r0:.4f}, N = 4 {r4:.4f}")
    assert r4 <= r0, (r4, r0)
