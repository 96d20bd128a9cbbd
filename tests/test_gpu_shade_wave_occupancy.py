"""k_shade_wave at five waves per SIMD (kernels.h) on a real MI355X: the rewritten group loop leaves every output as it was.

The kernel keeps one descriptor word per lane across shade_ray, addresses a group's rays from the group's first slot, parks the
per-chunk words (prefix, sample, seed, reference position) in LDS and runs ONE loop that screens while the queue holds fewer than 64
survivors and shades otherwise.  None of it may show.  Each case traces a small frame of the Cornell box twice on the GPU -- once
with k_shade_wave forced on from a given bounce (option shade_wave_from), once with k_shade for every bounce (shade_wave = 0) -- and
demands equal accumulator bytes and equal PolarisTraceStats (every field but the device time), and both equal to the per-sample sum of
the CPU oracle with the oracle's counters.

The shapes are the smallest that reach every path of the loop:

* 256 x 9, 4 spp, roulette from bounce 3, wave from bounce 3, prefilter on: 9 chunks a sample, 36 chunks in 4 full groups and one of 4
  (a partial group); after the roulette few rays survive the screen, so a group's queue is drained only at its end;
* the same with the prefilter off and the wave kernel from bounce 1: every ray is a survivor, a group of 8 full chunks sends up to
  2048 descriptors through a wave's ring of 128, which wraps, and the shade pass fires from inside the screening;
* 256 x 1, 2 spp: two chunks in all, num_chunks < 8, a group that ends inside the launch's only group;
* 250 x 3, 3 spp, roulette from bounce 1, wave from bounce 1: 750 paths in 768 slots (a padded last chunk), roulette played inside the
  wave kernel from its first bounce;
* the first case with the moments plane on (.w), and with the tables forced out of LDS (k_shade_wave<false>).
"""
import numpy as np
import pytest

from conftest import bits, make_hip_tracer
from test_gpu_parity import counters
from test_gpu_shade_prefilter import reference

pytestmark = pytest.mark.gpu

NB = 5
STAT_FIELDS = ("primary_rays", "indirect_rays", "occlusion_rays", "shaded_hits", "shaded_misses", "emitter_hits", "unoccluded")


def stats(st):
    """Every field of PolarisTraceStats but the device time."""
    return tuple(int(getattr(st, f)) for f in STAT_FIELDS) + (list(st.rays_per_bounce), list(st.occl_per_bounce))


def trace(sc, seeds, w, h, spp, rr, moments=False, **options):
    from oracle import pybind as ob

    tr = make_hip_tracer(sc, w, h, time_kernels=1, **options)
    try:
        if moments:
            tr.set_option("moments", 1)
        tr.Trace(ob.make_request(w, h, spp=spp, bounces=NB, rr=rr), seeds)
        launched = {t: tr.kernel_symbol(t) for t in ("shade_sort", "shade_plain", "shade_wave") if tr.kernel_ms(t)[1] > 0}
        return tr.read_accumulator(0), tr.last_trace_stats, launched
    finally:
        tr.Close()


# (id, width, height, spp, rr, wave from, prefilter, moments, further options)
CASES = [
    ("sparse-partial-group", 256, 9, 4, 3, 3, 1, False, {}),
    ("dense-ring-wraps", 256, 9, 4, 3, 1, 0, False, {}),
    ("two-chunks", 256, 1, 2, 3, 1, 1, False, {}),
    ("padded-chunk-roulette-inside", 250, 3, 3, 1, 1, 1, False, {}),
    ("moments", 256, 9, 4, 3, 3, 1, True, {}),
    ("tables-in-global-memory", 256, 9, 4, 3, 3, 1, False, {"stage_lds": 0}),
    ("tables-in-global-memory-dense", 256, 9, 4, 3, 1, 0, False, {"stage_lds": 0}),
]


@pytest.mark.parametrize("name,w,h,spp,rr,wave_from,prefilter,moments,more", CASES, ids=[c[0] for c in CASES])
def test_wave_kernel_equals_k_shade_and_the_oracle(built, oracle, name, w, h, spp, rr, wave_from, prefilter, moments, more):
    sc, seeds, _, ws, per_sample = reference(oracle, "cornell", rr, w, h, spp, NB)
    rays = list(ws.rays_per_bounce[:NB])
    if name == "dense-ring-wraps":
        # by counting: 36 chunks are 5 groups, so some group of bounce 1 holds more rays than a ring has entries -- and all are survivors
        assert rays[1] > 5 * 128, rays
    if name == "sparse-partial-group":
        assert 0 < rays[4] < rays[3] < rays[2], rays   # roulette thins bounces 3 and 4: the screen retires rays
    common = dict(more, shade_prefilter=prefilter)
    by_wave, wave_stats, wave_kernels = trace(sc, seeds, w, h, spp, rr, moments, shade_wave_from=wave_from, **common)
    by_chunk, chunk_stats, chunk_kernels = trace(sc, seeds, w, h, spp, rr, moments, shade_wave=0, **common)
    variant = "false" if more.get("stage_lds") == 0 else "true"
    assert wave_kernels.get("shade_wave") == f"pol::k_shade_wave<{variant}>", wave_kernels   # the kernel under test really ran ...
    assert "shade_wave" not in chunk_kernels, chunk_kernels                                   # ... and only in the first trace
    assert stats(wave_stats) == stats(chunk_stats), name
    assert np.array_equal(bits(by_wave), bits(by_chunk)), name
    assert counters(wave_stats, NB) == counters(ws, NB) and wave_stats.emitter_hits == ws.emitter_hits, name
    assert np.array_equal(bits(by_wave[..., :3]), bits(per_sample[..., :3])), name
    assert bool(by_wave[..., 3].any()) == moments, name
