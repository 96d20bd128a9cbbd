"""Which kernel runs under which options: the symbol every timer of a Trace brackets, pinned literally.

bench.py names its per-kernel roofline objects by the strings polaris_hip_kernel_symbol reports, so a string that drifts from
the template arguments really launched would price the wrong kernel without a failure anywhere.  Every expectation below is
written out -- derived from the selection rules in DESIGN.md 3.1 / 3.2, never read back from the library -- and each case also
traces the CPU oracle's frame (exact mode: bit for bit), so a variant that is selected is also a variant that works.

Frames of 64 x 48, 2 samples, 4 bounces, Russian roulette from bounce 2: the shade steps are first / sort / sort / wave by default.
"""
import os
import sys

import numpy as np
import pytest

from batched_oracle import per_sample_reference
from conftest import bits, make_hip_tracer
from test_gpu_parity import counters

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from stack_scenes import _nested_shells_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, B, RR = 64, 48, 2, 4, 2

GENERATE = "pol::k_generate"
PACKET_CAMERA, PACKET_ANY = "pol::k_trace_packet<false, true>", "pol::k_trace_packet<true, false>"
TINY_ONE = ("pol::k_trace<false, 16, 2, true>", "pol::k_trace<true, 16, 2, true>")
TINY_GENERAL = ("pol::k_trace<false, 16, 2, false>", "pol::k_trace<true, 16, 2, false>")
SHADE_LDS = {"shade_first": "pol::k_shade<true, false, true>", "shade_sort": "pol::k_shade<true, true, false>",
             "shade_plain": "pol::k_shade<true, false, false>", "shade_wave": "pol::k_shade_wave<true>"}
SHADE_GLOBAL = {"shade_first": "pol::k_shade<false, false, true>", "shade_sort": "pol::k_shade<false, true, false>",
                "shade_plain": "pol::k_shade<false, false, false>", "shade_wave": "pol::k_shade_wave<false>"}
SHADE_TIMERS = ("shade_first", "shade_sort", "shade_plain", "shade_wave")
TRACE_TIMERS = ("generate", "intersect", "intersect_packet", "occlusion") + SHADE_TIMERS + ("scan", "fold", "resolve")


def case(scene, options, intersect, occlusion, column=(0, 1, 1, 3), shade=SHADE_LDS, packet=False):
    """The timers a Trace of `scene` under `options` (exact mode) must bracket, with their symbols; every other timer of a Trace
    must report no launch.  intersect / occlusion: the symbol the timer ENDS on (its last bounce); column: the shade timer per bounce."""
    expect = {"generate": GENERATE, "intersect": intersect, "occlusion": occlusion}
    if packet:
        expect["intersect_packet"] = PACKET_CAMERA
    for t in sorted(set(column)):
        expect[SHADE_TIMERS[t]] = shade[SHADE_TIMERS[t]]
    return scene, options, expect, list(column)


CASES = {
    # the Cornell box is ONE instance whose boxes bound their subtrees: tiny-scene mode, ONE; its triangle records are in LDS, so camera rays take k_trace too
    "cornell-default": case("cornell", {}, *TINY_ONE),
    # several instances: tiny-scene mode, the general variant
    "cubes-default": case("cubes", {}, *TINY_GENERAL),
    # node records from global memory / the tree's top in LDS: 16-entry stack; camera rays of a small one-instance scene go through the packet kernel
    "cornell-lds-top": case("cornell", {"node_mode": 1}, "pol::k_trace<false, 16, 1, false>", "pol::k_trace<true, 16, 1, false>", packet=True),
    "cornell-global": case("cornell", {"node_mode": 0}, "pol::k_trace<false, 16, 0, false>", "pol::k_trace<true, 16, 0, false>", packet=True),
    "cornell-lds-top-packet": case("cornell", {"node_mode": 1, "packet_primary": 1}, "pol::k_trace<false, 16, 1, false>", "pol::k_trace<true, 16, 1, false>", packet=True),
    "cornell-global-packet": case("cornell", {"node_mode": 0, "packet_primary": 1}, "pol::k_trace<false, 16, 0, false>", "pol::k_trace<true, 16, 0, false>", packet=True),
    "cornell-global-no-packet": case("cornell", {"node_mode": 0, "packet_primary": 0}, "pol::k_trace<false, 16, 0, false>", "pol::k_trace<true, 16, 0, false>"),
    "cornell-tiny-packet": case("cornell", {"packet_primary": 1}, *TINY_ONE, packet=True),
    # shadow rays of the first bounce through the packet kernel: the occlusion timer ends on bounce 3's k_trace; of all four bounces: on the packet kernel
    "cornell-packet-shadow-1": case("cornell", {"packet_shadow": 1}, *TINY_ONE),
    "cornell-packet-shadow-4": case("cornell", {"packet_shadow": 4}, TINY_ONE[0], PACKET_ANY),
    # every camera ray holds 20 and more stack entries: the 24-entry stack
    "nested-shells": case("nested-shells", {"node_mode": 0, "max_leaf_tris": 0}, "pol::k_trace<false, 24, 0, false>", "pol::k_trace<true, 24, 0, false>", packet=True),
    # the plain formulation, one ray per lane
    "cornell-plain-traversal": case("cornell", {"traversal": 0}, "pol::k_intersect", "pol::k_occlusion"),
    # material / light / texture tables read from global memory
    "cornell-no-lds-tables": case("cornell", {"stage_lds": 0}, *TINY_ONE, shade=SHADE_GLOBAL),
    # the shade step per bounce
    "cornell-never-sorted": case("cornell", {"shade_sort": 32}, *TINY_ONE, column=(0, 2, 2, 3)),
    "cornell-no-wave": case("cornell", {"shade_wave": 0}, *TINY_ONE, column=(0, 1, 1, 1)),
    "cornell-wave-from-1": case("cornell", {"shade_wave_from": 1}, *TINY_ONE, column=(0, 3, 3, 3)),
}

_reference = {}


def make_request():
    from oracle import pybind as ob

    return ob.make_request(W, H, spp=SPP, bounces=B, rr=RR)


def reference(oracle, name):
    """(scene, seeds, the oracle's frame, its counters, the per-sample sum of the batched mode): once per scene, then shared unchanged."""
    from polaris_amd import scenes

    if name not in _reference:
        sc = _nested_shells_scene() if name == "nested-shells" else scenes.SCENES[name]()
        seeds = scenes.make_seeds(SPP, B, base=311)
        want, wst, _ = oracle.trace(sc, make_request(), seeds)
        assert wst.shaded_hits > 0 and wst.occlusion_rays > 0 and want[..., :3].sum() > 0, name   # (the comparison is not vacuous)
        per_sample, pst = per_sample_reference(oracle, sc, make_request, seeds, SPP, B)
        assert counters(pst, B) == counters(wst, B)
        for a in (want, per_sample):
            a.setflags(write=False)
        _reference[name] = (sc, seeds, want, wst, per_sample)
    return _reference[name]


def check_timers(tr, expect):
    """After a Trace: every expected timer ran and brackets the literal symbol; every other timer of a Trace did not run."""
    for name in TRACE_TIMERS:
        launches = tr.kernel_ms(name)[1]
        if name in expect:
            assert launches > 0, (name, "did not run")
            assert tr.kernel_symbol(name) == expect[name], (name, tr.kernel_symbol(name))
        elif name != "scan":
            assert launches == 0, (name, "ran", launches)
        else:
            assert launches > 0, "scan did not run"   # (one per bounce, whatever the options; it carries no pinned symbol)


@pytest.mark.parametrize("key", sorted(CASES))
def test_selected_kernels_in_exact_mode(built, oracle, key):
    name, options, expect, column = CASES[key]
    sc, seeds, want, wst, _ = reference(oracle, name)
    tr = make_hip_tracer(sc, W, H, exact_accumulate=1, time_kernels=1, **options)
    try:
        tr.Trace(make_request(), seeds)
        got, st = tr.read_accumulator(0), tr.last_trace_stats
        check_timers(tr, expect)      # (exact mode: neither fold nor resolve)
        assert [tr.SHADE_TIMERS.index(c["timer"]) for c in tr.shade_counts(B)] == column
    finally:
        tr.Close()
    assert counters(st, B) == counters(wst, B)
    assert np.array_equal(bits(got[..., :3]), bits(want[..., :3]))


def test_selected_kernels_in_batched_mode_with_moments(built, oracle):
    """The default mode adds the fold and the resolve; with moments the resolve is k_resolve<true> (where the timer names a symbol)."""
    sc, seeds, _, wst, per_sample = reference(oracle, "cornell")
    tr = make_hip_tracer(sc, W, H, time_kernels=1, moments=1)
    try:
        tr.Trace(make_request(), seeds)
        got, st = tr.read_accumulator(0), tr.last_trace_stats
        assert tr.kernel_symbol("resolve") in ("", "pol::k_resolve<true>")
        expect = dict(CASES["cornell-default"][2], fold="pol::k_fold_nee", resolve=tr.kernel_symbol("resolve"))
        check_timers(tr, expect)
        assert [tr.SHADE_TIMERS.index(c["timer"]) for c in tr.shade_counts(B)] == [0, 1, 1, 3]
    finally:
        tr.Close()
    assert counters(st, B) == counters(wst, B)
    assert np.array_equal(bits(got[..., :3]), bits(per_sample[..., :3]))
