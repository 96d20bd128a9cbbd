"""Exact hit ties, rays in box-face planes and the strict comparisons through every traversal kernel on a real MI355X.

DESIGN.md section 2 rests parity on one rule: the kernels traverse in their own order, order cannot change a minimum, and an EXACT
tie goes to the triangle the reference tests first (DFS rank; intersect.cl:281).  kernels.h writes that rule out five times --
traverse<> (k_intersect, k_occlusion, k_gbuffer), k_trace's big-leaf loop, its inline-leaf test_tri, the packet kernel, the tiny-mode
variants (TINY: packed rank | class | triangle words; ONE: no instance rank, one cull limit) -- over ranks scene_layout.h assigns.
The scenes of tests/tools/tie_scenes.py make every ray depend on it (their preconditions are counted on the CPU in
tests/test_tie_scenes_cpu.py; the oracle equals the compiled reference on them in tests/test_oracle_vs_reference.py).

Bar: hit flag, triangle (instance where a tap returns it) and the bits of (w, u, v, t) equal to the oracle's; whole frames bit-equal
with all ray counters equal.
"""
import os
import sys

import numpy as np
import pytest

import batched_oracle as BO
import motion_oracle as MO
from conftest import bits, make_hip_tracer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import tie_scenes as TS  # noqa: E402

pytestmark = pytest.mark.gpu

# the variants of test_gpu_probes.py::test_arbitrary_rays_through_every_traversal_kernel ...
VARIANTS = [dict(traversal=1, node_mode=m) for m in (0, 1, 2)] + [dict(traversal=0), dict(packet_primary=1, packet_shadow=32)]
VARIANTS += [dict(node_mode=2, lds_tris=0), dict(node_mode=2, lds_tris=37)]
VARIANTS += [dict(node_mode=2, tiny_one=0), dict(node_mode=2, tiny_one=0, lds_tris=37)]
LEAF_SPLITS = (0, 1, 2)   # ... each crossed with the upload's leaf subdivision (max_leaf_tris; 0 keeps the scene's own leaves)


class Want:
    """The oracle's answers for one scene and ray set, and for its shadow variants (maxDist at / one ulp below / above the hit)."""

    def __init__(self, oracle, sc, rays):
        self.sc, self.rays = sc, rays
        self.hit, self.wuvt, self.it = oracle.intersect(sc, rays, any_hit=False)
        self.occ, _, _ = oracle.intersect(sc, rays, any_hit=True)
        assert 0.2 < (self.hit != 0).mean() < 1.0
        self.shadow = {}
        for key, r in TS.shadow_variants(rays, self.hit, self.wuvt[:, 3]).items():
            self.shadow[key] = (r, oracle.intersect(sc, r, any_hit=True)[0], oracle.intersect(sc, r, any_hit=False))
        assert not self.shadow["at"][1].any() and self.shadow["above"][1].mean() > 0.9   # (a box's entry distance may round past t + 1 ulp)


def first_difference(got, want):
    d = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return (len(d), int(d[0]) if len(d) else -1)


def check_probes(tr, w, what):
    """probe_intersect closest / any hit and the shadow variants of `w` on an open tracer; count and first differing ray on failure."""
    hit, wuvt, tri = tr.probe_intersect(w.rays, any_hit=False)
    occ, _, _ = tr.probe_intersect(w.rays, any_hit=True)
    n, k = first_difference(hit, w.hit)
    assert n == 0, (what, "closest-hit flags", n, k, w.rays[k])
    h = w.hit != 0
    n, k = first_difference(tri[h], w.it[h, 1])
    assert n == 0, (what, "triangles", n, k, w.rays[h][k], int(tri[h][k]), int(w.it[h, 1][k]))
    n, k = first_difference(bits(wuvt[h]).reshape(-1), bits(w.wuvt[h]).reshape(-1))
    assert n == 0, (what, "wuvt words", n, k // 4, w.rays[h][k // 4])
    n, k = first_difference(occ, w.occ)
    assert n == 0, (what, "any-hit flags", n, k, w.rays[k])
    for key, (r, s_occ, (s_hit, s_wuvt, s_it)) in w.shadow.items():
        occ, _, _ = tr.probe_intersect(r, any_hit=True)
        n, k = first_difference(occ, s_occ)
        assert n == 0, (what, f"maxDist {key} t: any-hit flags", n, k, r[k])
        hit, wuvt, tri = tr.probe_intersect(r, any_hit=False)
        n, k = first_difference(hit, s_hit)
        assert n == 0, (what, f"maxDist {key} t: closest-hit flags", n, k, r[k])
        h = s_hit != 0
        assert np.array_equal(tri[h], s_it[h, 1]) and np.array_equal(bits(wuvt[h]), bits(s_wuvt[h])), (what, f"maxDist {key} t")


@pytest.mark.parametrize("tag", TS.CASES)
def test_tie_rays_through_every_traversal_kernel(built, oracle, tag):
    """Every scene of tie_scenes.CASES x the nine kernel variants x max_leaf_tris 0 / 1 / 2: closest hit, any hit and the three
    maxDist variants equal the oracle."""
    sc, rays = TS.case(tag)
    w = Want(oracle, sc, rays)
    for split in LEAF_SPLITS:
        for opts in VARIANTS:
            tr = make_hip_tracer(sc, 8, 8, max_leaf_tris=split, **opts)
            try:
                check_probes(tr, w, (tag, split, opts))
            finally:
                tr.Close()


@pytest.mark.parametrize("order", TS.ORDERS, ids=lambda o: "".join(map(str, o)))
def test_coincident_instances_by_instance_index(built, oracle, order):
    """Twins of ONE mesh differ in the instance index only, which probe_intersect does not return: the primary tap's (instance,
    triangle) equals the oracle's tap with the default selection, the one-ray-per-lane primary kernel and traversal = 0; and the
    INSTANCE plane of the first-hit G-buffer (k_gbuffer -> traverse<>; object_motion with temporal reuse on) equals
    oracle.intersect's instance on the centre rays (motion_oracle.gbuffer_inst)."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    W, H = 64, 48
    sc = TS.coincident_instances(order)
    seeds = scenes.make_seeds(1, 1, base=31)
    _, _, want = oracle.trace(sc, ob.make_request(W, H, spp=1, bounces=1, rr=2), seeds, tap_sample=0)
    h = want["primary_hit"] != 0
    twins = [g for grp in TS.SAME_MESH_TWINS for g in grp]
    assert np.isin(want["primary_tri"][h, 0], twins).sum() > 100 and np.isin(want["primary_tri"][h, 0], TS.DIFFERENT_MESH_TWINS).sum() > 100
    _, _, inst_want = MO.gbuffer_inst(oracle, sc, W, H)
    assert np.isin(inst_want, twins).sum() > 100
    for opts in ({}, {"packet_primary": 0}, {"traversal": 0}):
        tr = make_hip_tracer(sc, W, H, object_motion=1, **opts)
        try:
            got = tr.tap_primary(ob.make_request(W, H, spp=1, bounces=1, rr=2), int(seeds[0]))
            tr.set_temporal()
            inst = tr.read_instance_plane()
        finally:
            tr.Close()
        assert np.array_equal(got["primary_hit"] != 0, h), (order, opts)
        n, k = first_difference(got["primary_tri"][h].reshape(-1), want["primary_tri"][h].reshape(-1))
        assert n == 0, (order, opts, "primary (instance, triangle)", n, k // 2, got["primary_tri"][h][k // 2], want["primary_tri"][h][k // 2])
        assert np.array_equal(bits(got["primary_wuvt"][h]), bits(want["primary_wuvt"][h])), (order, opts)
        n, k = first_difference(inst.reshape(-1), inst_want.reshape(-1))
        assert n == 0, (order, opts, "INSTANCE plane", n, divmod(k, W))


@pytest.mark.parametrize("algorithm", ["sah", "lbvh"])
@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("tag", ["doubled-4-2", "lattice-4", "relief-4"])
def test_ties_in_device_built_trees(built, oracle, tag, max_leaf, algorithm):
    """Trees from the device builder number their nodes level by level: DFS rank is not array order.  The probes equal the oracle on
    the rebuilt arrays.  Printed, not asserted: how often the winner of a doubled pair has the HIGHER scene index (with compile_scene
    trees: never).  Measured on an MI355X: 0 of 18 405 hits for sah and lbvh, max_leaf_tris 1 and 4 -- the builder hands the triangles
    back in the order of its leaves, so the lower index is still the first reached."""
    from polaris_amd import bvh_build

    sc0, rays = TS.case(tag)
    sc, _ = bvh_build.rebuild_on_device(sc0, max_leaf_tris=max_leaf, algorithm=algorithm)
    w = Want(oracle, sc, rays)
    if tag.startswith("doubled"):
        twin = TS.twin_of(sc)
        win = w.it[w.hit != 0, 1]
        print(f"{tag} {algorithm} max_leaf_tris={max_leaf}: the winner has the higher scene index of its pair in {(win > twin[win]).mean():.4f} of {len(win)} hits")
    for opts in VARIANTS:
        tr = make_hip_tracer(sc, 8, 8, **opts)
        try:
            check_probes(tr, w, (tag, algorithm, max_leaf, opts))
        finally:
            tr.Close()


def counters(st, B):
    return (list(st.rays_per_bounce[:B]), list(st.occl_per_bounce[:B]), st.primary_rays, st.indirect_rays, st.occlusion_rays,
            st.shaded_hits, st.shaded_misses, st.unoccluded, st.emitter_hits)


@pytest.mark.parametrize("tag", ["doubled-4-2", "doubled-split-4-5", "coincident-012", "coincident-021", "lattice-4", "relief-4"])
def test_whole_frames_of_tie_scenes(built, oracle, tag):
    """One 64 x 48 frame, 2 spp, 3 bounces: exact mode bit-equal to oracle.trace with all ray counters equal; the default batched
    mode equal to batched_oracle.sum_ascending."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    W, H, spp, B = 64, 48, 2, 3
    sc, _ = TS.case(tag)
    seeds = scenes.make_seeds(spp, B, base=53)
    make_req = lambda: ob.make_request(W, H, spp=spp, bounces=B)  # noqa: E731
    want, st, _ = oracle.trace(sc, make_req(), seeds)
    assert want[..., :3].any() and st.occlusion_rays > 0 and st.unoccluded > 0 and st.shaded_hits > 0
    batched, bst = BO.per_sample_reference(oracle, sc, make_req, seeds, spp, B)
    for opts, ref, rst in (({"exact_accumulate": 1}, want, st), ({}, batched, bst)):
        tr = make_hip_tracer(sc, W, H, **opts)
        try:
            tr.Trace(make_req(), seeds)
            got, gs = tr.read_accumulator(0), tr.last_trace_stats
        finally:
            tr.Close()
        assert counters(gs, B) == counters(rst, B), (tag, opts)
        differing = int((bits(got[..., :3]) != bits(ref[..., :3])).sum())
        assert differing == 0, (tag, opts, f"{differing} accumulator words differ")
