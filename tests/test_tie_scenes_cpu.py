"""The preconditions of the tie tests (tests/tools/tie_scenes.py), on the CPU oracle and an independent statement -- never on HIP.

tests/test_gpu_ties.py holds every traversal kernel to the oracle on scenes built so that an exact tie, a ray in a box-face plane or a
strict comparison decides the answer.  That pins something only if the inputs really are what they claim: here the claims are counted.
The independent statement is a float32 Moeller-Trumbore over ALL triangles in array order (tie_scenes.brute_force: no tree, numpy
arithmetic); the winner among tied triangles is restated by a plain left-first depth-first walk of sc.bvh_nodes.

Measured (asserted below with margins):
  lattice, max_leaf 1 / 2 / 4 / 10: 48.7 / 48.7 / 51.4 / 52.6 % of the hits are exact ties; 147 / 147 / 175 / 189 hit rays tie six ways;
      16.9 / 16.9 / 13.5 / 11.8 % of all rays are brute-force hits the reference's traversal drops (0 * inf = NaN in the slab test);
  relief (vertex heights 0 .. 3), max_leaf 1 / 4 / 20: 30.2 / 32.9 / 36.9 % of the hits are exact ties, 116 / 119 / 158 six ways, 16.6 / 13.5 /
      8.5 % of the rays dropped; the leaves' boxes have 4 / 3 / 3 different tops;
  doubled: 92.0 % of the rays hit, every hit a two-way tie, the winner the twin reached first by the walk (the lower scene index) in 100 %;
      split variants: on 11.6 % of the hits the winner sits in the subtree a near-child-first traversal enters second;
  coincident instances: same-mesh twins go to the first of the walk of the top tree (instances 3 and 5); different-mesh twins go to the
      mesh whose outrigger lies at -x, whatever its index: instance 1 over instance 0 in orders (0, 1, 2) and (2, 1, 0), instance 2 over
      0 and 1 in order (0, 2, 1) (4 495 hits each); in order (1, 2, 0) it is instance 0;
  epsilon edges: 199 of 400 (t > 1e-5f) and 200 of 400 (|det| >= 1e-5f) hit, none on a zero-area triangle; maxDist == t: 0 % occluded,
      one ulp more: 100 %.
"""
import os
import sys

import numpy as np
import pytest

from conftest import bits

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import tie_scenes as TS  # noqa: E402


def _brute_agrees(oracle, sc, rays):
    """The brute force agrees with the oracle's t bits on every hit of the oracle (which it must also hit).  -> (hit mask, wuvt,
    inst_tri, brute winner, multiplicity)."""
    h, wuvt, it = oracle.intersect(sc, rays)
    hm = h != 0
    bt, bw, bm = TS.brute_force(sc, rays)
    assert hm.any() and (bw[hm] >= 0).all()
    assert np.array_equal(bits(bt[hm]), bits(wuvt[hm, 3]))
    return hm, wuvt, it, bw, bm


@pytest.mark.parametrize("max_leaf", TS.LATTICE_LEAVES)
def test_lattice_rays_tie_and_run_in_box_planes(oracle, max_leaf):
    sc, rays = TS.case(f"lattice-{max_leaf}")
    assert len(rays) == 9583 and sc.num_triangles == 128 and len(sc.mesh_instances) == 1
    hm, wuvt, it, bw, bm = _brute_agrees(oracle, sc, rays)
    assert set(np.unique(wuvt[hm, 3]).tolist()) <= {1.0, 2.0, 4.0}          # every t is exact
    ties = float((bm[hm] >= 2).mean())
    six = int((bm[hm] == 6).sum())
    dropped = float(((bw >= 0) & ~hm).mean())
    print(f"lattice max_leaf={max_leaf}: ties {ties:.4f} of {int(hm.sum())} hits, six-way {six}, dropped {dropped:.4f} of {len(rays)} rays")
    assert ties >= 0.40
    assert six > 0
    assert dropped >= 0.05                                                 # brute-force hits the traversal misses: the NaN slab path


def test_the_larger_lattices_keep_their_preconditions(oracle):
    """The 40 x 40 lattice exceeds the tiny-scene modes' 2 046 triangle slots whatever the leaf size; the big-leaf lattice has leaves
    of more than 15 triangles."""
    sc, rays = TS.case("lattice-40")
    assert sc.num_triangles == 3200 > 2046 and len(rays) <= 40000
    h, _, _ = oracle.intersect(sc, rays)
    assert 0.5 < (h != 0).mean() < 0.95
    sc, rays = TS.case("lattice-big-leaf")
    leaf = (sc.bvh_nodes["ldata"] <= 0) & (sc.bvh_nodes["rdata"] > 0)
    assert int(sc.bvh_nodes["rdata"][leaf].max()) > 15
    hm, _, _, bw, bm = _brute_agrees(oracle, sc, rays)
    assert (bm[hm] >= 2).mean() >= 0.40 and ((bw >= 0) & ~hm).mean() >= 0.05


@pytest.mark.parametrize("max_leaf", TS.RELIEF_LEAVES)
def test_relief_rays_tie_across_boxes_entered_at_different_distances(oracle, max_leaf):
    """The lattice with vertex heights 0 .. 3: the surface folds over itself along the slanted rays, so the nearest brute-force hit may
    be one the traversal drops (the oracle then reports a farther one, never a nearer); where both report the same distance the bits
    agree.  Ties (exact: det = +-1 under the vertical rays) now join triangles whose leaves' boxes differ."""
    sc, rays = TS.case(f"relief-{max_leaf}")
    assert len(rays) == 9583 and sc.num_triangles == 128 and len(sc.mesh_instances) == 1
    z = sc.vertices[:, 2]
    assert set(np.unique(z).tolist()) == {0.0, 1.0, 2.0, 3.0} and z.reshape(-1, 3)[(sc.vertices[:, 0] <= 3).reshape(-1, 3).all(axis=1)].max() <= 1.0
    h, wuvt, it = oracle.intersect(sc, rays)
    hm = h != 0
    bt, bw, bm = TS.brute_force(sc, rays)
    assert (bw[hm] >= 0).all() and (bt[hm] <= wuvt[hm, 3]).all()
    same = bits(bt[hm]) == bits(wuvt[hm, 3])
    ties, six, dropped = float((bm[hm][same] >= 2).mean()), int((bm[hm][same] == 6).sum()), float(((bw >= 0) & ~hm).mean())
    boxes = sc.bvh_nodes[(sc.bvh_nodes["ldata"] <= 0) & (sc.bvh_nodes["rdata"] > 0)]
    print(f"relief max_leaf={max_leaf}: nearest hit kept {same.mean():.4f}, ties {ties:.4f} of those, six-way {six}, dropped {dropped:.4f}, "
          f"{len(np.unique(boxes['max'][:, 2]))} distinct leaf-box tops")
    assert same.mean() >= 0.95 and ties >= 0.20 and six > 0 and dropped >= 0.05
    assert len(np.unique(boxes["max"][:, 2])) >= 2     # a vertical ray enters the leaves of one tie at different distances


@pytest.mark.parametrize("tag", [c for c in TS.CASES if c.startswith("doubled")])
def test_doubled_every_hit_is_a_tie_won_by_the_first_in_walk_order(oracle, tag):
    sc, rays = TS.case(tag)
    assert sc.num_triangles == 184 and len(rays) == 20000
    hm, wuvt, it, bw, bm = _brute_agrees(oracle, sc, rays)
    assert hm.mean() >= 0.90
    assert (bm[hm] >= 2).all()
    twin = TS.twin_of(sc)
    assert (twin >= 0).all() and (sc.material_index != sc.material_index[twin]).all()      # a wrong winner is another material
    order = TS.dfs_triangle_order(sc)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    win = it[hm, 1]
    assert (rank[win] < rank[twin[win]]).all()
    assert np.array_equal(win, bw[hm])                                                      # array order == walk order for these trees
    assert (win < twin[win]).all()
    if "split" in tag:
        # the first copies of the sphere are the left child of the mesh root, everything else the right one, whose box is the room: a
        # ray that starts inside the room and outside the sphere's box is in the right box before it enters the left one -- and its
        # sphere hit goes to the LEFT twin
        root = sc.bvh_nodes[int(sc.mesh_instances[0]["bvh_root"])]
        left, right = sc.bvh_nodes[int(root["ldata"])], sc.bvh_nodes[int(root["rdata"])]
        n_left = len(TS.dfs_triangle_order(sc, int(root["ldata"])))
        o = rays[hm, 0:3]
        inside = lambda b: ((o >= b["min"]) & (o <= b["max"])).all(axis=1)  # noqa: E731
        second = (win < n_left) & inside(right) & ~inside(left)
        print(f"{tag}: the winner sits in the subtree a near-first traversal enters second on {second.mean():.4f} of {len(win)} hits")
        assert n_left == 80 and second.mean() >= 0.05


def test_coincident_instances_go_to_the_first_of_the_top_trees_walk(oracle):
    higher = {}
    for order in TS.ORDERS:
        sc = TS.coincident_instances(order)
        rays = TS.coincident_rays()
        h, wuvt, it = oracle.intersect(sc, rays)
        hm = h != 0
        walk = TS.dfs_instance_order(sc)
        assert sorted(walk) == list(range(len(sc.mesh_instances)))
        pos = {inst: k for k, inst in enumerate(walk)}
        count = np.bincount(it[hm, 0], minlength=len(sc.mesh_instances))
        for group in TS.SAME_MESH_TWINS:                                     # same mesh, same transform: every hit of the group is a tie
            first = min(group, key=pos.get)
            assert count[first] > 1000 and all(count[g] == 0 for g in group if g != first), (order, group, count)
        # different meshes: the cube's twelve triangles tie three ways; only the outriggers belong to one instance alone
        first = min(TS.DIFFERENT_MESH_TWINS, key=pos.get)
        others = [g for g in TS.DIFFERENT_MESH_TWINS if g != first]
        assert count[first] > 1000 and sum(count[g] for g in others) <= 0.01 * count[first], (order, count)
        outriggers = np.nonzero(np.abs(sc.vertices[:, 0].reshape(-1, 3)).max(axis=1) == 4.0)[0]
        assert len(outriggers) == 2
        for g in others:                                                      # what the others win are their outriggers
            assert np.isin(it[hm & (it[:, 0] == g), 1], outriggers).all(), (order, g)
        higher[order] = int(count[first]) if any(g < first for g in others) else 0
    print("hits won by the higher instance index of tied different-mesh twins:", higher)
    assert max(higher.values()) > 1000


@pytest.mark.parametrize("max_leaf", TS.EPSILON_LEAVES)
def test_epsilon_edges_sit_on_both_sides_of_the_strict_comparisons(oracle, max_leaf):
    sc = TS.epsilon_edges(max_leaf)
    zero = TS.zero_area_triangles(sc)
    assert len(zero) == 2 and sc.num_triangles == 4
    for name, (rays, k) in (("t", TS.epsilon_t_rays()), ("det", TS.epsilon_det_rays())):
        assert len(rays) == 400
        hm, wuvt, it, bw, bm = _brute_agrees(oracle, sc, rays)
        assert 0.40 <= hm.mean() <= 0.60, (name, hm.mean())
        assert np.array_equal(hm, k > 0 if name == "t" else k >= 0)          # the strict comparison, restated on the ray's construction
        assert not np.isin(it[hm, 1], zero).any() and (bm[hm] == 2).all()
        sv = TS.shadow_variants(rays, hm, wuvt[:, 3])
        for key, want in (("at", 0.0), ("below", 0.0), ("above", 1.0)):
            occ, _, _ = oracle.intersect(sc, sv[key], any_hit=True)
            hit, _, _ = oracle.intersect(sc, sv[key], any_hit=False)
            assert float((occ != 0).mean()) == want and float((hit != 0).mean()) == want, (name, key)
