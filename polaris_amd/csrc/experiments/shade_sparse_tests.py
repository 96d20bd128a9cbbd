"""GPU tests of the closed k_shade_sparse experiment (shade_sparse.diff): NOT part of the suite, the product does not hold the kernel.

To run them: build the variant (scripts/build_variant.sh sparse --patch shade_sparse), copy this file to tests/test_gpu_shade_sparse.py
and run it with POLARIS_HIP_LIB set to the library that script prints (pytest -m gpu tests/test_gpu_shade_sparse.py).
All its cases passed on an MI355X when the experiment was closed (profiles/shade_sparse_ab.txt, section 1).

k_shade_sparse (kernels.h): the roulette bounces shaded by chunk group -- screen, compact, then sort -- on a real MI355X.

One workgroup takes a group of 8 consecutive chunks: it screens the group's live rays (shade_fate), queues the survivors'
descriptors in (chunk, slot) order and shades them in rounds of 256, each round in class order.  The bars are those of
test_gpu_shade_prefilter.py, whose references and checks are used as they are:

* exact mode is BIT-IDENTICAL to the CPU oracle's accumulator,
* batched mode is BIT-IDENTICAL to the per-sample sum,
* in both every counter of test_gpu_parity.counters() plus emitter_hits equals the oracle's,

with the prefilter on and off, and the two equal to each other.  Every case forces the kernel with shade_sparse_from=1 (by
default it serves only launches of many groups per CU; the last test pins that rule).
"""
import numpy as np
import pytest

from conftest import bits, make_hip_tracer
from test_gpu_parity import counters
from test_gpu_shade_prefilter import B, H, SPP, W, check, hip_trace, reference

pytestmark = pytest.mark.gpu

SPARSE = {"shade_sparse_from": 1}
GROUP = 8                # kernels.h, kSparseShadeGroup
MIN_GROUPS_PER_CU = 8    # trace_plan.h, kSparseMinGroupsPerCu: the automatic rule's launch size


def both_prefilters(ref, rr, opts, exact, what, **shape):
    off = check(ref, rr, dict(opts, shade_prefilter=0), exact, (what, exact, "off"), **shape)
    on = check(ref, rr, dict(opts, shade_prefilter=1), exact, (what, exact, "on"), **shape)
    assert np.array_equal(bits(off), bits(on)), (what, exact)
    return on


@pytest.mark.parametrize("shape", [(8, 8, 6, 5), (300, 1, 6, 5), (96, 80, 6, 12)], ids=lambda s: "x".join(map(str, s)))
def test_group_and_round_edges(built, oracle, shape):
    """One partly filled chunk; two chunks of one group, the second with 44 slots; 180 chunks in 23 groups, the last of 4 chunks,
    groups straddling samples.  The big frame runs 12 bounces so that its last bounces are nearly empty."""
    w, h, spp, nb = shape
    rr = 1
    ref = reference(oracle, "cornell", rr, w, h, spp, nb)
    ws = ref[3]
    if (w, h) == (96, 80):
        # From the counters, by counting: every ray of bounce b + 1 has a parent that survived the screen of bounce b (prefilter on or
        # off), so more than 256 x groups of them mean a group whose queue is longer than one round -- and then some round boundary
        # cuts a chunk's survivors in two, because a group's queue is in (chunk, slot) order and a chunk holds at most 256.
        chunks = spp * ((w * h + 255) // 256)
        groups = (chunks + GROUP - 1) // GROUP
        assert (chunks, groups, chunks % GROUP) == (180, 23, 4)
        rays = list(ws.rays_per_bounce[:nb])
        assert any(rays[b + 1] > 256 * groups for b in range(1, nb - 1)), "no group is sure to shade more than one round"
        assert any(0 < rays[b] < groups for b in range(1, nb)), "no bounce is sure to leave a group without a live ray"
    for exact in (True, False):
        both_prefilters(ref, rr, SPARSE, exact, shape, w=w, h=h, spp=spp, nb=nb)


@pytest.mark.parametrize("rr", [0, 1, 3, 5])
@pytest.mark.parametrize("name", ["cornell", "sphere", "many-materials", "materials"])
def test_wherever_roulette_starts(built, oracle, name, rr):
    """Every bounce after the first through the kernel, roulette from bounce 0, 1, 3 and 5 (nowhere): an open box, an environment light
    (misses are shaded, nothing escapes), more reach sets than classes (class 15 is shared) and textured operators."""
    ref = reference(oracle, name, rr)
    for exact in (True, False):
        both_prefilters(ref, rr, SPARSE, exact, (name, rr))


def test_an_emitter_behind_a_mix(built, oracle):
    """Every wall class can emit: roulette retires nothing there and the groups run many rounds with the prefilter on.  Not vacuous:
    the oracle counts emitter hits at bounces >= min_rr (all its emitter hits less those of the camera rays, which a one-bounce trace
    with the same camera and first shade seeds counts), and some ray was rejected."""
    from oracle import pybind as ob

    rr = 1
    ref = reference(oracle, "glowing-walls", rr)
    sc, seeds, _, ws, _ = ref
    first = np.ascontiguousarray(np.asarray(seeds, np.uint32).reshape(SPP, 1 + B)[:, :2])  # per sample: camera seed, shade seed of bounce 0
    _, s0, _ = oracle.trace(sc, ob.make_request(W, H, spp=SPP, bounces=1, rr=rr), first.reshape(-1))
    assert s0.rays_per_bounce[0] == ws.rays_per_bounce[0]
    assert ws.emitter_hits - s0.emitter_hits > 0, "no emitter hit at a roulette bounce: the case checks nothing"
    assert ws.rays_per_bounce[1] - ws.rays_per_bounce[2] > ws.emitter_hits, "no ray was rejected"
    for exact in (True, False):
        both_prefilters(ref, rr, SPARSE, exact, "glowing-walls")


OPTION_SETS = [{"stage_lds": 0}, {"samples_per_batch": 1}, {"samples_per_batch": 4}, {"overlap": 3}, {"shade_sort": 32}]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", ["cornell", "many-materials"])
def test_option_sets(built, oracle, name, opts):
    """Tables in global memory, batch sizes, batches in flight and unsorted k_shade in front of the kernel.  (samples_per_batch and
    overlap shape batched traces only.)"""
    rr = 3
    ref = reference(oracle, name, rr)
    batched_only = "samples_per_batch" in opts or "overlap" in opts
    for exact in ((False,) if batched_only else (True, False)):
        both_prefilters(ref, rr, dict(SPARSE, **opts), exact, (name, opts))


def test_determinism_with_four_batches_in_flight(built, oracle):
    """The same Trace five times on one handle, four pipelines: equal bits every time (and the oracle's)."""
    rr = 3
    ref = reference(oracle, "cornell", rr)
    sc, seeds, _, ws, per_sample = ref
    runs = hip_trace(sc, seeds, rr, dict(SPARSE, overlap=4, samples_per_batch=1), repeat=5)
    for got, gs in runs:
        assert counters(gs, B) == counters(ws, B) and gs.emitter_hits == ws.emitter_hits
        assert np.array_equal(bits(got), bits(runs[0][0]))
    assert np.array_equal(bits(runs[0][0][..., :3]), bits(per_sample[..., :3]))


def test_forced_selection(built, oracle):
    """shade_sparse_from=1 at the frame of test_gpu_kernel_selection.py: every bounce after the first reports timer shade_wave, and the
    timer brackets the sparse kernel."""
    import test_gpu_kernel_selection as sel

    sc, seeds, want, wst, _ = sel.reference(oracle, "cornell")
    tr = make_hip_tracer(sc, sel.W, sel.H, exact_accumulate=1, time_kernels=1, **SPARSE)
    try:
        tr.Trace(sel.make_request(), seeds)
        got, st = tr.read_accumulator(0), tr.last_trace_stats
        assert [tr.SHADE_TIMERS.index(c["timer"]) for c in tr.shade_counts(sel.B)] == [0, 3, 3, 3]
        assert tr.kernel_symbol("shade_wave") == "pol::k_shade_sparse<true>"
        assert tr.kernel_ms("shade_sort")[1] == 0 and tr.kernel_ms("shade_plain")[1] == 0
    finally:
        tr.Close()
    assert counters(st, sel.B) == counters(wst, sel.B)
    assert np.array_equal(bits(got[..., :3]), bits(want[..., :3]))


def test_automatic_selection_by_launch_size(built, oracle):
    """Defaults, batched mode, a 512 x 512 frame (128 groups a sample), roulette from bounce 1 of 3: a Trace whose full batch has
    MIN_GROUPS_PER_CU groups per CU takes the sparse kernel at the roulette bounces, one sample less per batch keeps k_shade_wave
    (roulette bounce itself: k_shade SORT).  Both equal the per-sample sum."""
    w = h = 512
    nb, rr = 3, 1
    probe = make_hip_tracer(reference(oracle, "cornell", 3)[0], W, H)
    try:
        cus = probe.device_cus
    finally:
        probe.Close()
    groups_per_sample = w * h // 256 // GROUP
    k = -(-MIN_GROUPS_PER_CU * cus // groups_per_sample)  # samples per batch at the threshold
    assert k >= 2 and k * groups_per_sample >= cus
    ref = reference(oracle, "cornell", rr, w, h, k, nb)
    sc, seeds, _, ws, per_sample = ref
    from oracle import pybind as ob

    for per_batch, column, symbol in ((k, [0, 3, 3], "pol::k_shade_sparse<true>"), (k - 1, [0, 1, 3], "pol::k_shade_wave<true>")):
        tr = make_hip_tracer(sc, w, h, time_kernels=1, samples_per_batch=per_batch)
        try:
            tr.Trace(ob.make_request(w, h, spp=k, bounces=nb, rr=rr), seeds)
            got, gs = tr.read_accumulator(0), tr.last_trace_stats
            assert [tr.SHADE_TIMERS.index(c["timer"]) for c in tr.shade_counts(nb)] == column, per_batch
            assert tr.kernel_symbol("shade_wave") == symbol, (per_batch, tr.kernel_symbol("shade_wave"))
        finally:
            tr.Close()
        assert counters(gs, nb) == counters(ws, nb) and gs.emitter_hits == ws.emitter_hits, per_batch
        assert np.array_equal(bits(got[..., :3]), bits(per_sample[..., :3])), per_batch
