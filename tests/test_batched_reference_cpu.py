"""The per-sample reference of the default (batched) mode on the CPU (no GPU): tests/batched_oracle.py proves itself against the
oracle's own full trace, and the bit-exact bar it sets is shown to tell apart what the RMSE <= 1e-6 bar cannot -- the same terms summed
in the reference's order, in descending sample order, or as two batches added pairwise all stay within 1e-6 of it and all differ from it
in thousands of accumulator words."""
import numpy as np
import pytest

import batched_oracle as BO
import variance_oracle as VO
from conftest import bits

F = np.float32
W, H, SPP, B = 96, 80, 6, 5
SCENES = ["cornell", "cubes", "materials"]


def rmse(a, b, spp):
    return float(np.sqrt(np.mean((a[..., :3] / spp - b[..., :3] / spp) ** 2)))


def counters(st, nb):
    return (list(st.rays_per_bounce[:nb]), list(st.occl_per_bounce[:nb]), st.primary_rays, st.indirect_rays, st.occlusion_rays,
            st.shaded_hits, st.shaded_misses, st.unoccluded, st.emitter_hits)


@pytest.fixture(scope="module", params=SCENES)
def case(request, oracle):
    from oracle import pybind as ob
    from polaris_amd import scenes

    sc = scenes.SCENES[request.param]()
    seeds = scenes.make_seeds(SPP, B, base=1234)

    def make_req():
        return ob.make_request(W, H, spp=SPP, bounces=B)

    full, fst, _ = oracle.trace(sc, make_req(), seeds)
    frames, total = BO.per_sample_frames(oracle, sc, make_req, seeds, SPP, B)
    ref, rst = BO.per_sample_reference(oracle, sc, make_req, seeds, SPP, B)
    return dict(name=request.param, sc=sc, seeds=seeds, make_req=make_req, full=full, fst=fst, frames=frames, total=total, ref=ref, rst=rst)


def test_one_sample_traces_walk_the_full_traces_paths(case):
    """The six one-sample traces' counters sum to the full trace's: the same paths, the seed slices are the right ones."""
    assert counters(case["total"], B) == counters(case["fst"], B)
    assert counters(case["rst"], B) == counters(case["fst"], B)
    assert case["fst"].primary_rays == W * H * SPP and case["fst"].occlusion_rays > 0


def test_reference_is_the_ascending_float32_sum(case):
    acc = np.zeros((H, W, 3), F)
    for x in case["frames"]:
        acc = acc + x[..., :3]
    assert acc.dtype == F
    assert np.array_equal(bits(case["ref"][..., :3]), bits(acc))
    assert not case["ref"][..., 3].any()


def test_old_bar_holds_for_the_reference_itself(case):
    """RMSE against the oracle's reference-order accumulator <= 1e-6: the bar the GPU tests keep beside the new one."""
    err = rmse(case["ref"], case["full"], SPP)
    print(f"{case['name']}: per-sample sum vs reference order: rmse {err:.3e}")
    assert err <= 1e-6


def test_bit_equality_discriminates_where_the_rmse_bar_cannot(case):
    """(a) the reference-order accumulator, (b) the samples summed in descending order, (c) two batches of three summed first and then
    added: each within RMSE 1e-6 of the helper's result -- the old bar passes all three -- and each different from it in more than 100
    accumulator words: np.array_equal(bits(..)) fails for every one of them."""
    ref, frames = case["ref"], case["frames"]
    desc = BO.sum_ascending(frames[::-1], ref.shape)
    pair = BO.sum_ascending(frames[:3], ref.shape) + BO.sum_ascending(frames[3:], ref.shape)
    for what, other in (("reference order", case["full"]), ("descending", desc), ("two batches pairwise", pair)):
        differing = int((bits(other[..., :3]) != bits(ref[..., :3])).sum())
        err = rmse(other, ref, SPP)
        print(f"{case['name']}: {what}: {differing} of {ref[..., :3].size} words differ, rmse {err:.3e}")
        assert err <= 1e-6, what
        assert differing > 100, what
        assert not np.array_equal(bits(other[..., :3]), bits(ref[..., :3])), what


def test_moments_plane_and_zero_samples(case, oracle):
    """.w = sum of lum(L_k)^2 in ascending k with moments (0 without), .xyz the same either way; spp = 0 gives zeros and no rays."""
    sc, make_req, seeds = case["sc"], case["make_req"], case["seeds"]
    m, mst = BO.per_sample_reference(oracle, sc, make_req, seeds, SPP, B, moments=True)
    assert np.array_equal(bits(m[..., :3]), bits(case["ref"][..., :3]))
    w = np.zeros((H, W), F)
    for x in case["frames"]:
        lx = VO.lum(x[..., :3])
        w = w + lx * lx
    assert np.array_equal(bits(m[..., 3]), bits(w)) and (w > 0).mean() > 0.5
    assert counters(mst, B) == counters(case["fst"], B)
    z, zst = BO.per_sample_reference(oracle, sc, make_req, seeds, 0, B, moments=True)
    assert z.shape == (H, W, 4) and z.dtype == F and not bits(z).any()
    assert zst.primary_rays == 0 and zst.total_rays() == 0


def test_row_block_and_fresh_requests(oracle):
    """A partial row block: rows outside it stay zero, the request handed out is not the one traced (sample count untouched)."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    sc = scenes.SCENES["cubes"]()
    w, h, by, bh, spp, nb = 70, 9, 4, 2, 3, 4
    seeds = scenes.make_seeds(spp, nb)
    made = []

    def make_req():
        made.append(ob.make_request(w, h, spp=spp, bounces=nb, block_y=by, block_h=bh))
        return made[-1]

    ref, st = BO.per_sample_reference(oracle, sc, make_req, seeds, spp, nb)
    full, fst, _ = oracle.trace(sc, ob.make_request(w, h, spp=spp, bounces=nb, block_y=by, block_h=bh), seeds)
    assert len(made) == spp + 1 and len({id(r) for r in made}) == spp + 1
    assert counters(st, nb) == counters(fst, nb) and st.primary_rays == w * bh * spp
    assert not ref[:by].any() and not ref[by + bh:].any() and ref[by:by + bh, :, :3].any()
    assert rmse(ref, full, spp) <= 1e-6
