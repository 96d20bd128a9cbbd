"""Which kernel shades the bounce where Russian roulette starts: the automatic shade_wave_from by launch size, on a real MI355X.

With the prefilter a chunk of the first roulette bounce keeps about a sixth of its live rays, and k_shade_wave -- persistent waves
that screen and shade a group of 8 chunks at a time -- beats k_shade's workgroup per chunk there, on launches large enough to keep its
grid busy (profiles/shade_sparse_ab.txt).  polaris_hip.hip, plan_bounces: k_shade_wave starts at min_bounces_for_rr instead of
min_bounces_for_rr + 1 when the prefilter is on, some shading class of the scene cannot emit, and a full batch of the Trace holds at
least GROUPS_PER_CU groups per compute unit.  Everything smaller keeps the plan that test_gpu_kernel_selection.py pins.

The expectations are written out from that rule, never read back from the library, and every Trace here is also bit-equal to the
per-sample sum of the CPU oracle with the oracle's counters: a kernel that is selected is a kernel that works.
"""
import numpy as np
import pytest

from conftest import bits, make_hip_tracer
from test_gpu_parity import counters
from test_gpu_shade_prefilter import reference

pytestmark = pytest.mark.gpu

GROUP = 8            # kernels.h, kSparseGroup: chunks of 256 slots per group
GROUPS_PER_CU = 8    # polaris_hip.hip, kWaveRouletteGroupsPerCu
W = H = 512          # 1024 chunks = 128 groups a sample
NB, RR = 3, 1        # roulette from bounce 1 of 3: bounce 1 is the roulette bounce
SORT_THEN_WAVE, WAVE_FROM_ROULETTE = [0, 1, 3], [0, 3, 3]


def samples_at_threshold(cus):
    groups_per_sample = W * H // 256 // GROUP
    return -(-GROUPS_PER_CU * cus // groups_per_sample)


def trace(sc, seeds, spp, **options):
    from oracle import pybind as ob

    tr = make_hip_tracer(sc, W, H, time_kernels=1, **options)
    try:
        cus = tr.device_cus
        tr.Trace(ob.make_request(W, H, spp=spp, bounces=NB, rr=RR), seeds)
        column = [tr.SHADE_TIMERS.index(c["timer"]) for c in tr.shade_counts(NB)]
        symbols = {t: tr.kernel_symbol(t) for t in ("shade_sort", "shade_wave") if tr.kernel_ms(t)[1] > 0}
        return tr.read_accumulator(0), tr.last_trace_stats, column, symbols, cus
    finally:
        tr.Close()


@pytest.fixture(scope="module")
def case(built, oracle):
    """(samples per batch at the threshold, the reference of a Trace of that many samples): computed once."""
    probe = make_hip_tracer(reference(oracle, "cornell", 3)[0], 96, 80)
    try:
        k = samples_at_threshold(probe.device_cus)
    finally:
        probe.Close()
    assert 2 <= k <= 64, k   # (16 on the MI355X's 256 compute units)
    return k, reference(oracle, "cornell", RR, W, H, k, NB)


PLANS = [
    ("at-threshold", 0, {}, WAVE_FROM_ROULETTE),
    ("one-sample-below", -1, {}, SORT_THEN_WAVE),
    ("prefilter-off", 0, {"shade_prefilter": 0}, SORT_THEN_WAVE),
    ("wave-from-given", 0, {"shade_wave_from": RR + 1}, SORT_THEN_WAVE),
    ("no-wave", 0, {"shade_wave": 0}, [0, 1, 1]),
]


@pytest.mark.parametrize("name,delta,options,column", PLANS, ids=[p[0] for p in PLANS])
def test_roulette_bounce_by_launch_size(case, name, delta, options, column):
    """One batch of k samples is at the threshold, batches of k - 1 (the last one holds the remaining sample) are below it; the
    prefilter off, or an explicit shade_wave_from, keep the earlier plan whatever the size."""
    k, (sc, seeds, _, ws, per_sample) = case
    got, gs, col, symbols, cus = trace(sc, seeds, k, samples_per_batch=k + delta, **options)
    assert (k + delta) * (W * H // 256 // GROUP) >= GROUPS_PER_CU * cus if name == "at-threshold" else True
    assert col == column, (name, col)
    if 3 in column:
        assert symbols["shade_wave"] == "pol::k_shade_wave<true>", symbols
    if 1 in column:
        assert symbols["shade_sort"] == "pol::k_shade<true, true, false>", symbols
    assert counters(gs, NB) == counters(ws, NB) and gs.emitter_hits == ws.emitter_hits, name
    assert np.array_equal(bits(got[..., :3]), bits(per_sample[..., :3])), name


def test_the_sphere_scene_takes_the_rule_too(case, oracle):
    """An environment light (misses are shaded, nothing escapes) over a scene whose shading classes do not all emit: the rule reads the
    scene's classes, the prefilter and the launch size, nothing else -- the same plan at the same size, equal to the oracle."""
    k, _ = case
    sc, seeds, _, ws, per_sample = reference(oracle, "sphere", RR, W, H, k, NB)
    got, gs, col, symbols, _ = trace(sc, seeds, k, samples_per_batch=k)
    assert col == WAVE_FROM_ROULETTE and symbols["shade_wave"] == "pol::k_shade_wave<true>", (col, symbols)
    assert counters(gs, NB) == counters(ws, NB) and gs.emitter_hits == ws.emitter_hits
    assert np.array_equal(bits(got[..., :3]), bits(per_sample[..., :3]))
