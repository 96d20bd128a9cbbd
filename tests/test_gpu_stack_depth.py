"""Every traversal kernel at the limits of its node stack on a real MI355X: scenes that need exactly 15, 16 | 17, 24 | 25, 31 and 32
entries (tests/tools/stack_scenes.py), and 33, which the upload refuses.

DESIGN.md section 3.1 ("The stack contract"): scene_layout.h promises max_stack, select_trace picks k_trace<*, 16 | 24 | 32, *> from
it, plan_tiny_lds lays out exactly the tiny mode's 16-bit rows, traverse<> and the packet kernel keep 32 entries.  A row miscounted
anywhere faults nowhere: it lands in LDS that belongs to the work cursor, the staged tree, another lane's column -- and only the rays
at the deep end get a wrong hit.  tests/test_stack_scenes_cpu.py counts that at least 32 rays of every case hold the most entries the
layout allows, in the traversal order each kernel uses; tests/test_oracle_vs_reference.py holds the oracle to the compiled reference
on the same inputs.

Bar: everything is compared bit for bit or literally -- hit flags, triangles, the words of (w, u, v, t), accumulators, ray counters,
G-buffer planes, and the symbols the timers bracket, written out from the selection rules of DESIGN.md 3.1 and never read back.
"""
import os
import sys

import numpy as np
import pytest

import batched_oracle as BO
import gbuffer_oracle as G
import motion_oracle as MO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_ties import check_probes, counters

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import stack_scenes as SS  # noqa: E402
import tie_scenes as TS  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, B, RR = 32, 24, 2, 3, 2
PROBE_OPTIONS = [{}, {"node_mode": 0}, {"node_mode": 1}, {"node_mode": 2}, {"node_mode": 2, "tiny_one": 0}, {"node_mode": 2, "lds_tris": 0},
                 {"traversal": 0}, {"packet_primary": 1, "packet_shadow": 32}]
FRAME_OPTIONS = [{}, {"node_mode": 0}, {"node_mode": 1}, {"node_mode": 2}, {"traversal": 0}, {"packet_shadow": 4}]
PACKET_CAMERA, PACKET_ANY = "pol::k_trace_packet<false, true>", "pol::k_trace_packet<true, false>"


class Want:
    """test_gpu_ties.Want for these rays: the oracle's answers for one scene and ray set and for its shadow variants.  (A local copy:
    the shells' leaf boxes are flat, a ray enters them AT the hit distance, and that entry may round past t + 1 ulp -- the original asks
    that 90 % of the `above` rays be occluded, here it is some of them.)"""

    def __init__(self, oracle, sc, rays):
        self.sc, self.rays = sc, rays
        self.hit, self.wuvt, self.it = oracle.intersect(sc, rays, any_hit=False)
        self.occ, _, _ = oracle.intersect(sc, rays, any_hit=True)
        assert 0.2 < (self.hit != 0).mean() < 1.0 and 0 < (self.occ != 0).sum() < len(rays)
        self.shadow = {}
        for key, r in TS.shadow_variants(rays, self.hit, self.wuvt[:, 3]).items():
            self.shadow[key] = (r, oracle.intersect(sc, r, any_hit=True)[0], oracle.intersect(sc, r, any_hit=False))
        assert not self.shadow["at"][1].any() and not self.shadow["below"][1].any() and self.shadow["above"][1].any()


_cache = {}


def reference(oracle, tag):
    """{scene, rays, want (probes), frame, stats, per_sample, per_sample_stats} of a case: computed once, then shared unchanged."""
    from polaris_amd import scenes

    if tag not in _cache:
        sc, rays = SS.case(tag)
        seeds = scenes.make_seeds(SPP, B, base=61)
        frame, st, _ = oracle.trace(sc, make_request(), seeds)
        assert st.shaded_hits > 0 and st.occlusion_rays > 0 and st.unoccluded > 0 and frame[..., :3].sum() > 0 and st.rays_per_bounce[B - 1] > 0, tag
        per_sample, pst = BO.per_sample_reference(oracle, sc, make_request, seeds, SPP, B)
        assert counters(pst, B) == counters(st, B)
        for a in (rays, frame, per_sample, seeds):
            a.setflags(write=False)
        _cache[tag] = dict(sc=sc, rays=rays, seeds=seeds, want=Want(oracle, sc, rays), frame=frame, st=st, per_sample=per_sample)
    return _cache[tag]


def make_request():
    from oracle import pybind as ob

    return ob.make_request(W, H, spp=SPP, bounces=B, rr=RR)


def expected_symbols(tag, opts):
    """{timer: symbol} of the three traversal timers of a Trace of `tag` under `opts` (exact mode), from the rules of DESIGN.md 3.1 --
    a timer that is absent must not have run.  intersect / occlusion: the symbol the timer ENDS on (its last bounce).

    * tiny-scene mode (NODES = 2, STACK = 16) where the layout needs <= 16 entries; asked for elsewhere, it is dropped, and the scene
      gets what it gets by default: the tree's top in LDS (NODES = 1; these trees have a few dozen pair records);
    * STACK = 16 | 24 | 32 from max_stack <= 16 | <= 24 | else;
    * ONE where the tiny mode runs a scene that is one instance (whose boxes bound their subtrees);
    * camera rays go through the packet kernel in a one-instance scene unless the tiny mode holds its triangle records in LDS (it
      holds all of these); shadow rays of the first packet_shadow bounces too."""
    c = SS.CASES[tag]
    S, one_instance = c["S"], c["family"] == "single"
    tiny_ok = S <= 16
    nodes = opts.get("node_mode", -1)
    if nodes < 0 or (nodes == 2 and not tiny_ok):
        nodes = 2 if tiny_ok else 1
    tiny = nodes == 2
    stack = 16 if S <= 16 else (24 if S <= 24 else 32)
    one = "true" if tiny and one_instance and opts.get("tiny_one", 1) else "false"
    out = {"intersect": f"pol::k_trace<false, {stack}, {nodes}, {one}>", "occlusion": f"pol::k_trace<true, {stack}, {nodes}, {one}>"}
    if not opts.get("traversal", 1):
        out = {"intersect": "pol::k_intersect", "occlusion": "pol::k_occlusion"}
    if one_instance and not tiny:
        out["intersect_packet"] = PACKET_CAMERA
    if opts.get("packet_shadow", 0) >= B:
        out["occlusion"] = PACKET_ANY
    return out


def test_expected_symbols_spell_out_the_rules():
    """(the table's own corners, so that a slip in expected_symbols() cannot hide behind the library's answer)"""
    assert expected_symbols("single-16", {}) == {"intersect": "pol::k_trace<false, 16, 2, true>", "occlusion": "pol::k_trace<true, 16, 2, true>"}
    assert expected_symbols("instanced-16", {}) == {"intersect": "pol::k_trace<false, 16, 2, false>", "occlusion": "pol::k_trace<true, 16, 2, false>"}
    assert expected_symbols("single-15", {"node_mode": 0}) == {"intersect": "pol::k_trace<false, 16, 0, false>", "occlusion": "pol::k_trace<true, 16, 0, false>", "intersect_packet": PACKET_CAMERA}
    assert expected_symbols("instanced-17", {"node_mode": 2}) == {"intersect": "pol::k_trace<false, 24, 1, false>", "occlusion": "pol::k_trace<true, 24, 1, false>"}
    assert expected_symbols("single-24-mirror", {}) == {"intersect": "pol::k_trace<false, 24, 1, false>", "occlusion": "pol::k_trace<true, 24, 1, false>", "intersect_packet": PACKET_CAMERA}
    assert expected_symbols("single-25", {"node_mode": 0}) == {"intersect": "pol::k_trace<false, 32, 0, false>", "occlusion": "pol::k_trace<true, 32, 0, false>", "intersect_packet": PACKET_CAMERA}
    assert expected_symbols("instanced-32", {"packet_shadow": 4}) == {"intersect": "pol::k_trace<false, 32, 1, false>", "occlusion": PACKET_ANY}
    assert expected_symbols("single-31", {"traversal": 0}) == {"intersect": "pol::k_intersect", "occlusion": "pol::k_occlusion", "intersect_packet": PACKET_CAMERA}


@pytest.mark.parametrize("tag", SS.TRACED)
def test_probes_through_every_traversal_kernel(built, oracle, tag):
    """probe_intersect closest hit, any hit and the three maxDist variants equal the oracle under every option set."""
    ref = reference(oracle, tag)
    for opts in PROBE_OPTIONS:
        tr = make_hip_tracer(ref["sc"], 8, 8, max_leaf_tris=0, **opts)
        try:
            check_probes(tr, ref["want"], (tag, opts))
        finally:
            tr.Close()


@pytest.mark.parametrize("tag", SS.TRACED)
def test_frames_and_the_selected_symbols(built, oracle, tag):
    """One 32 x 24 frame in exact mode per option set: the oracle's accumulator bit for bit, all ray counters equal, and the traversal
    timers bracket the literal symbols the stack need selects."""
    ref = reference(oracle, tag)
    for opts in FRAME_OPTIONS:
        tr = make_hip_tracer(ref["sc"], W, H, exact_accumulate=1, time_kernels=1, max_leaf_tris=0, **opts)
        try:
            tr.Trace(make_request(), ref["seeds"])
            got, st = tr.read_accumulator(0), tr.last_trace_stats
            ran = {name: tr.kernel_symbol(name) for name in ("intersect", "occlusion", "intersect_packet") if tr.kernel_ms(name)[1] > 0}
        finally:
            tr.Close()
        print(f"{tag} {opts}: {ran}")
        assert ran == expected_symbols(tag, opts), (tag, opts, ran)
        assert counters(st, B) == counters(ref["st"], B), (tag, opts)
        differing = int((bits(got[..., :3]) != bits(ref["frame"][..., :3])).sum())
        assert differing == 0, (tag, opts, f"{differing} accumulator words differ")


@pytest.mark.parametrize("tag", SS.TRACED)
def test_batched_mode(built, oracle, tag):
    """The default mode: the per-sample sum of tests/batched_oracle.py bit for bit, all ray counters equal."""
    ref = reference(oracle, tag)
    tr = make_hip_tracer(ref["sc"], W, H, max_leaf_tris=0)
    try:
        tr.Trace(make_request(), ref["seeds"])
        got, st = tr.read_accumulator(0), tr.last_trace_stats
    finally:
        tr.Close()
    assert counters(st, B) == counters(ref["st"], B), tag
    differing = int((bits(got[..., :3]) != bits(ref["per_sample"][..., :3])).sum())
    assert differing == 0, (tag, f"{differing} accumulator words differ")


@pytest.mark.parametrize("tag", SS.TRACED)
def test_first_hit_gbuffer(built, oracle, tag):
    """GUIDE, ALBEDO and INSTANCE (k_gbuffer: traverse<> over its fixed 32 entries) equal the oracle's first hits bit for bit."""
    ref = reference(oracle, tag)
    want_g, want_a, want_i = MO.gbuffer_inst(oracle, ref["sc"], W, H)
    assert (want_g[..., 3] < G.FLT_MAX).sum() > W * H // 2
    tr = make_hip_tracer(ref["sc"], W, H, object_motion=1, time_kernels=1, max_leaf_tris=0)
    try:
        guide, albedo = tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        tr.set_temporal()
        inst = tr.read_instance_plane()
        assert tr.kernel_symbol("gbuffer") == "pol::k_gbuffer"
    finally:
        tr.Close()
    for name, got, want in (("GUIDE", guide, want_g), ("ALBEDO", albedo, want_a), ("INSTANCE", inst, want_i)):
        differing = int((bits(got) != bits(want)).sum())
        assert differing == 0, (tag, name, f"{differing} words differ")


@pytest.mark.parametrize("tag", SS.REFUSED)
def test_a_need_of_33_entries_is_refused_and_the_handle_lives_on(built, oracle, tag):
    """The upload of a scene that needs 33 entries fails and says so; the same handle then takes the family's 32-entry scene and
    traces it bit for bit."""
    from polaris_amd.tracer import ChangeType, HipTracer, TracerError, UpdateMode

    deep, _ = SS.case(tag)
    ref = reference(oracle, tag.replace("33", "32"))
    tr = HipTracer("stack", 0)
    tr.Init()
    try:
        for k, v in (("exact_accumulate", 1), ("max_leaf_tris", 0)):
            tr.set_option(k, v)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (W, H))
        with pytest.raises(TracerError) as e:
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, deep)
        assert "traversal stack of 33 entries" in str(e.value), str(e.value)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, ref["sc"])
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, ref["sc"])
        tr.Trace(make_request(), ref["seeds"])
        got, st = tr.read_accumulator(0), tr.last_trace_stats
    finally:
        tr.Close()
    assert counters(st, B) == counters(ref["st"], B)
    assert np.array_equal(bits(got[..., :3]), bits(ref["frame"][..., :3]))


def test_retry_without_subdivision(built, oracle):
    """`retry` uploaded with max_leaf_tris = 1: subdividing its twelve-triangle leaf would need more than 32 entries, the upload falls
    back to the unsplit tree, and every option set answers the probes as the oracle does."""
    ref = reference(oracle, "retry")
    for opts in PROBE_OPTIONS:
        tr = make_hip_tracer(ref["sc"], 8, 8, max_leaf_tris=1, **opts)
        try:
            check_probes(tr, ref["want"], ("retry", "max_leaf_tris=1", opts))
        finally:
            tr.Close()
