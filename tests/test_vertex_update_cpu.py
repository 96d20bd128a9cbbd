"""CPU tests of deforming meshes in place (polaris_hip_update_vertices; polaris_amd/csrc/vertex_update.h).

tests/tools/vertex_update_check.cpp applies the HOST RESTATEMENT of the update -- the mesh plan build_layout keeps, the argument checks,
the triangle records, the mesh refit, then the instance update's own restatement, the very functions the kernels are made of -- to
build_layout(base).  The bars:

  max_leaf_tris = 0   the triangle, pair and instance records are byte-equal to build_layout(refit)'s.  A scene of at most 2 046 slots
                      orders its slots by the area of their leaf's box, which deforms: there the update keeps the uploaded order, and
                      the records are compared with every triangle-leaf reference resolved to the scene triangles it names and the
                      triangle records matched by scene triangle.
  max_leaf_tris 2, 4  the topology leaf subdivision added is kept, so records are not comparable one to one.  Every triangle record
                      equals the refit layout's for its scene triangle; every node of the caller's tree has refit.bvh_nodes[node] and
                      the cull factor 1.001 in its parent's pair record; every added box is the fold of the triangles below it -/+ the
                      padding, which is bit-equal to the padding build_layout(refit) computes for that mesh.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vertex_update_cases as cases
from conftest import ROOT
from polaris_amd import ctypes_api as T
from polaris_amd import scenes
from test_instance_update_cpu import TRI_RECORD, Records, resolved

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "vertex_update_check.cpp")
LIB = os.path.join(BUILD, "libvertex_update_check.so")
CAP = 1 << 22
PLAN_NODE = np.dtype([("a", "<i4"), ("b", "<i4"), ("count", "<u4"), ("pair_side", "<i4"), ("padded", "<i4"), ("mesh", "<u4"), ("node", "<u4"), ("first_tri", "<u4")])
PADDED_BOX = np.dtype([("pair", "<i4"), ("side_mesh", "<u4"), ("lo", "<f4", 3), ("hi", "<f4", 3)])
E_BAD_ARGUMENT, E_BAD_SCENE, E_UNSUPPORTED = 2, 5, 6
F32 = np.float32
CULL = np.float32(1.001).tobytes()


@pytest.fixture(scope="module")
def tool():
    os.makedirs(BUILD, exist_ok=True)
    csrc = os.path.join(ROOT, "polaris_amd", "csrc")
    deps = [SRC, os.path.join(ROOT, "include", "polaris_hip.h")] + [os.path.join(csrc, h) for h in ("scene_layout.h", "instance_update.h", "vertex_update.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, SRC, "-o", LIB])
    return C.CDLL(LIB)


def layout(tool, sc, max_leaf):
    """((pairs, insts, tris), pads per mesh) of build_layout(sc)."""
    r, view = Records(), T.scene_view(sc)
    pads = np.zeros(64, F32)
    rc = tool.vu_layout(C.byref(view), max_leaf, *r.args(), C.c_void_p(pads.ctypes.data), 64, r.err, C.c_size_t(512))
    assert rc == 0, r.err.value.decode()
    return r.take(), pads


class Updated:
    """build_layout(base) with the restated update `u` applied: records, status, message, the mesh plan and the update's paddings."""

    def __init__(self, tool, base, max_leaf, u, option_on=True):
        r, view = Records(), T.scene_view(base)
        status, sizes = C.c_int(0), np.zeros(5, np.uint32)
        nodes, slot_src, padded, pads = np.zeros(CAP, np.uint8), np.zeros(CAP // 4, np.uint32), np.zeros(CAP, np.uint8), np.zeros(64, F32)
        rc = tool.vu_update(C.byref(view), max_leaf, int(option_on), C.byref(u) if u is not None else None, *r.args(), C.byref(status),
                            C.c_void_p(sizes.ctypes.data), C.c_void_p(nodes.ctypes.data), C.c_void_p(slot_src.ctypes.data), C.c_void_p(padded.ctypes.data),
                            C.c_void_p(pads.ctypes.data), r.err, C.c_size_t(512))
        assert rc == 0, r.err.value.decode()
        self.records, self.status, self.msg, self.sizes = r.take(), status.value, r.err.value.decode(), sizes
        self.nodes = nodes[:int(sizes[0]) * 32].view(PLAN_NODE).copy()
        self.slot_src = slot_src[:len(self.records[2])].copy()
        self.padded = padded[:int(sizes[3]) * 32].view(PADDED_BOX).copy()
        self.pads = pads[:int(sizes[2])].copy()


def by_triangle(tris):
    return {int(t["orig"]) & 0xFFFFFF: t.tobytes() for t in tris}


def fold(vertices, tri_list):
    """The fold rule over the triangles `tri_list`, in order, of each v0, v1, v2."""
    v = vertices[(3 * np.asarray(tri_list)[:, None] + np.arange(3)).reshape(-1), :3]
    lo, hi = v[0].copy(), v[0].copy()
    for b in v[1:]:
        lo = np.where(b < lo, b, lo)
        hi = np.where(b > hi, b, hi)
    return lo, hi


def triangles_below(up, i):
    """Scene triangles below plan node i, left subtree first, a leaf's in its own order."""
    n = up.nodes[i]
    if n["count"] and n["b"] < 0:
        return [int(t) for t in up.slot_src[int(n["a"]):int(n["a"]) + int(n["count"])]]
    return triangles_below(up, int(n["a"])) + triangles_below(up, int(n["b"]))


# ---- 1. max_leaf_tris = 0: the records of a full layout ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_restated_update_equals_layout_of_refit_scene(tool, name):
    base, refit, _ = cases.case(name)
    (want, _), (before, _) = layout(tool, refit, 0), layout(tool, base, 0)
    u, keep = T.vertex_update(*cases.update_args(name))
    up = Updated(tool, base, 0, u)
    got = up.records
    assert up.status == 0, up.msg
    assert up.sizes[4] == 1 and up.sizes[3] == 0 and up.sizes[0] > 0
    assert before[2].tobytes() != got[2].tobytes(), "the case deforms nothing"
    assert got[1].tobytes() == want[1].tobytes(), "instance records"
    if got[2].tobytes() == want[2].tobytes():
        assert got[0].tobytes() == want[0].tobytes(), "pair records"
    else:   # the slot order of a tiny scene followed the leaf areas (module docstring)
        assert len(got[2]) <= 2046 and by_triangle(got[2]) == by_triangle(want[2]), "triangle records, matched by scene triangle"
        assert resolved(got[0], got[2]) == resolved(want[0], want[2]), "pair records, leaf references resolved"
    if name == "grid-64":
        assert up.sizes[0] > 1024 and len(got[2]) > 2046     # a launch per level on the device; not tiny: byte equality above
    if name == "big-leaves":
        assert (up.nodes["count"] > 15).any()
    if name == "cornell":
        assert base.num_triangles == 808 and len(base.mesh_instances) == 1
    if name == "panel-light":
        one_leaf = up.nodes[(up.nodes["count"] > 0) & (up.nodes["b"] < 0) & (up.nodes["pair_side"] < 0)]
        assert len(one_leaf) == 2                          # the panel and the floor: mesh roots that are leaves, no pair record holds their boxes
    if name == "reader-boxes":
        cull = np.concatenate([got[0]["cull0"], got[0]["cull1"]])
        assert np.isinf(cull).any() and np.array_equal(np.isinf(cull), np.isinf(np.concatenate([before[0]["cull0"], before[0]["cull1"]])))
    if name == "collapsed":   # a leaf that holds +0 and -0 side by side, and zero-extent boxes in the records
        y = refit.vertices[:, 1]
        leaves = up.nodes[(up.nodes["count"] > 0) & (up.nodes["b"] < 0)]
        mixed = 0
        for n in leaves:
            ys = np.concatenate([y[3 * t:3 * t + 3] for t in up.slot_src[int(n["a"]):int(n["a"]) + int(n["count"])]])
            mixed += bool((ys == 0).all() and np.signbit(ys).any() and not np.signbit(ys).all())
        assert mixed > 0
        assert ((got[0]["lo0"][:, 1] == got[0]["hi0"][:, 1]) & (got[0]["hi0"][:, 1] == 0)).any()


# ---- 2. leaf subdivision on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [2, 4])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_with_leaf_subdivision_boxes_and_padding_follow(tool, name, max_leaf):
    base, refit, _ = cases.case(name)
    (want, want_pads), _ = layout(tool, refit, max_leaf), None
    u, keep = T.vertex_update(*cases.update_args(name))
    up = Updated(tool, base, max_leaf, u)
    pairs, insts, tris = up.records
    assert up.status == 0, up.msg
    assert by_triangle(tris) == by_triangle(want[2]), "triangle records, matched by scene triangle"
    assert insts["r0"].tobytes() == want[1]["r0"].tobytes() and insts["r1"].tobytes() == want[1]["r1"].tobytes() and insts["r2"].tobytes() == want[1]["r2"].tobytes()
    assert up.pads.tobytes() == want_pads[:len(up.pads)].tobytes(), "the padding of every mesh equals the full layout's"
    NN = len(base.bvh_nodes)
    added = 0
    for i, n in enumerate(up.nodes):
        if n["pair_side"] < 0:
            continue
        p, side = pairs[int(n["pair_side"]) >> 1], int(n["pair_side"]) & 1
        lo, hi, cull = p["lo1" if side else "lo0"], p["hi1" if side else "hi0"], p["cull1" if side else "cull0"]
        assert cull.tobytes() == CULL, int(n["node"])
        if n["node"] < NN:
            ref = refit.bvh_nodes[int(n["node"])]
            assert lo.tobytes() == ref["min"].tobytes() and hi.tobytes() == ref["max"].tobytes(), int(n["node"])
        else:
            added += 1
            flo, fhi = fold(refit.vertices, triangles_below(up, i))
            pad = up.pads[int(n["mesh"])]
            assert up.padded[int(n["padded"])]["lo"].tobytes() == flo.tobytes() and up.padded[int(n["padded"])]["hi"].tobytes() == fhi.tobytes()
            assert lo.tobytes() == (flo - pad).astype(F32).tobytes() and hi.tobytes() == (fhi + pad).astype(F32).tobytes(), int(n["node"])
    assert added == up.sizes[3]
    if name == "big-leaves" or (max_leaf == 2 and name in ("cornell", "grid-64")):   # (the scenes' own leaves hold up to 4, big-leaves' up to 20)
        assert added > 0


# ---- 3. refit_vertices against a plain loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moving-and-deformed", "collapsed", "panel-light"])
def test_refit_vertices_equals_a_plain_bottom_up_loop(name):
    base, refit, _ = cases.case(name)
    nodes = base.bvh_nodes.copy()

    def fit(i):
        n = nodes[i]
        if n["ldata"] <= 0:
            first, count = -int(n["ldata"]), int(n["rdata"])
            nodes["min"][i], nodes["max"][i] = fold(refit.vertices, list(range(first, first + count)))
            return
        l, r = int(n["ldata"]), int(n["rdata"])
        fit(l)
        fit(r)
        a, b = nodes["min"][l], nodes["min"][r]
        nodes["min"][i] = np.where(b < a, b, a)
        a, b = nodes["max"][l], nodes["max"][r]
        nodes["max"][i] = np.where(b > a, b, a)

    roots = sorted(set(int(r) for r in base.mesh_instances["bvh_root"]))
    for root in roots:
        fit(root)
    mesh_level = np.ones(len(nodes), dtype=bool)
    mesh_level[scenes._top_level_nodes(base)[0]] = False
    assert refit.bvh_nodes[mesh_level].tobytes() == nodes[mesh_level].tobytes()
    assert refit.bvh_nodes[mesh_level].tobytes() != base.bvh_nodes[mesh_level].tobytes()
    again = scenes.refit_instances(refit, refit)             # the top level is a fixed point of refit_instances
    assert again.bvh_nodes.tobytes() == refit.bvh_nodes.tobytes()
    area = refit.emissives["type"] == T.EMISSIVE_AREA
    for e in np.nonzero(area)[0]:
        p = refit.vertices[3 * int(refit.emissives["tri_index"][e]):3 * int(refit.emissives["tri_index"][e]) + 3, :3].astype(np.float64)
        assert refit.emissives["area"][e] == F32(0.5 * np.linalg.norm(np.cross(p[2] - p[0], p[2] - p[1])))
    if name == "panel-light":
        assert (refit.emissives["area"][area] != base.emissives["area"][area]).any()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def shared_subtree_scene():
    """instanced_cubes(2) with a copy of the cube's root node as a second mesh root for instance 2: two roots, one pair of subtrees."""
    sc = scenes.instanced_cubes(2)
    root = int(sc.mesh_instances["bvh_root"][2])
    assert sc.bvh_nodes["ldata"][root] > 0 and (sc.mesh_instances["bvh_root"] == root).sum() > 1
    out = scenes.refit_instances(sc, sc)
    out.bvh_nodes = np.concatenate([sc.bvh_nodes, sc.bvh_nodes[root:root + 1]])
    out.mesh_instances["bvh_root"][2] = len(sc.bvh_nodes)
    return out, int(sc.bvh_nodes["ldata"][root])


def _refusals(name="moving-and-deformed"):
    """(what, status, text, (update, keep), option on) of every refusal the host decides."""
    base, refit, _ = cases.case(name)
    vertices, boxes, normals, inv, ems = scenes.vertex_update_args(refit)
    NI = len(inv)

    def edit(arr, fn):
        a = arr.copy()
        fn(a)
        return a

    def nan_vertex(a): a[7, 1] = np.nan
    def big_vertex(a): a[4, 2] = np.float32(2.0 ** 40 * 1.0001)
    def nan_entry(a): a[1, 5] = np.nan
    def big_entry(a): a[NI - 1, 12] = np.float32(2.0 ** 30 * 1.0001)
    def inf_box(a): a[0, 4] = np.inf
    def flipped_box(a): a[1, 0], a[1, 3] = a[1, 3] + 1.0, a[1, 0]
    def other_triangle(a): a["tri_index"][0] += 1
    def other_type(a): a["type"][0] = T.EMISSIVE_ENVIRONMENT
    def other_node(a): a["mat_node_index"][0] += 1

    def with_field(uk, field, value):
        setattr(uk[0], field, value)
        return uk

    mk = T.vertex_update
    yield "option off", E_UNSUPPORTED, "vertex_update off", mk(vertices, boxes, normals, inv, ems), False
    yield "struct_size", E_BAD_ARGUMENT, "struct_size", with_field(mk(vertices, boxes, normals, inv, ems), "struct_size", C.sizeof(T.VertexUpdate) + 8), True
    yield "triangle count", E_BAD_ARGUMENT, "triangles, the uploaded scene has", mk(vertices[:-3], boxes, None, inv, ems), True
    yield "instance count", E_BAD_ARGUMENT, "mesh instances, the uploaded scene has", mk(vertices, boxes[:-1], normals, None, ems), True
    yield "null vertices", E_BAD_ARGUMENT, "pointer is null", with_field(mk(vertices, boxes, normals, inv, ems), "vertices", None), True
    yield "null boxes", E_BAD_ARGUMENT, "pointer is null", with_field(mk(vertices, boxes, normals, inv, ems), "instance_boxes", None), True
    yield "emissive count", E_BAD_ARGUMENT, "emissives, the uploaded scene has", mk(vertices, boxes, normals, inv, np.concatenate([ems, ems[:1]])), True
    yield "emissive triangle", E_BAD_ARGUMENT, "differs from the uploaded one", mk(vertices, boxes, normals, inv, edit(ems, other_triangle)), True
    yield "emissive type", E_BAD_ARGUMENT, "differs from the uploaded one", mk(vertices, boxes, normals, inv, edit(ems, other_type)), True
    yield "emissive material node", E_BAD_ARGUMENT, "differs from the uploaded one", mk(vertices, boxes, normals, inv, edit(ems, other_node)), True
    yield "NaN vertex", E_BAD_SCENE, "triangle 2: vertex coordinate not finite or beyond 2^40", mk(edit(vertices, nan_vertex), boxes, normals, inv, ems), True
    yield "vertex beyond 2^40", E_BAD_SCENE, "triangle 1: vertex coordinate not finite or beyond 2^40", mk(edit(vertices, big_vertex), boxes, normals, inv, ems), True
    yield "NaN matrix entry", E_BAD_SCENE, "mesh instance 1: matrix entry not finite or beyond 2^30", mk(vertices, boxes, normals, edit(inv, nan_entry), ems), True
    yield "matrix entry beyond 2^30", E_BAD_SCENE, "matrix entry not finite or beyond 2^30", mk(vertices, boxes, normals, edit(inv, big_entry), ems), True
    yield "infinite box", E_BAD_SCENE, "mesh instance 0: box not finite or min > max", mk(vertices, edit(boxes, inf_box), normals, inv, ems), True
    yield "box min > max", E_BAD_SCENE, "mesh instance 1: box not finite or min > max", mk(vertices, edit(boxes, flipped_box), normals, inv, ems), True


def test_refusals_return_their_status_and_text_and_change_nothing(tool):
    """Each refusal returns its status with its message, and the restatement has touched no record when it refuses.  That a refused
    call leaves a TRACER as it was is shown on the device (tests/test_gpu_vertex_update.py)."""
    base, refit, _ = cases.case("moving-and-deformed")
    untouched, _ = layout(tool, base, 2)
    for what, status, text, (u, keep), option_on in _refusals():
        up = Updated(tool, base, 2, u, option_on)
        assert up.status == status and text in up.msg, (what, up.status, up.msg)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(up.records, untouched)), what
    up = Updated(tool, base, 2, None)
    assert up.status == E_BAD_ARGUMENT and "null" in up.msg
    good, keep = T.vertex_update(*scenes.vertex_update_args(refit))          # (the same arguments unedited are accepted)
    up = Updated(tool, base, 2, good)
    assert up.status == 0 and up.records[2].tobytes() != untouched[2].tobytes()


def test_shared_subtree_uploads_and_is_refused_by_name(tool):
    sc, shared_node = shared_subtree_scene()
    (records, _) = layout(tool, sc, 2)                                       # the layout itself is fine
    u, keep = T.vertex_update(*scenes.vertex_update_args(sc))
    up = Updated(tool, sc, 2, u)
    assert up.sizes[4] == 0 and up.status == E_UNSUPPORTED
    assert "no mesh plan was kept" in up.msg and "shared by two mesh trees" in up.msg
    assert f"BVH node {shared_node} " in up.msg or f"BVH node {shared_node + 1} " in up.msg
    assert all(a.tobytes() == b.tobytes() for a, b in zip(up.records, records))


def test_ctypes_mirror_matches_the_header():
    assert C.sizeof(T.VertexUpdate) == 64 and T.VertexUpdate().struct_size == 64
    assert "polaris_hip_update_vertices" in T.C_ABI_SYMBOLS
