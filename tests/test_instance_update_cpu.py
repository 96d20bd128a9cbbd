"""CPU tests of moving mesh instances in place (polaris_hip_update_instances; polaris_amd/csrc/instance_update.h).

tests/tools/instance_update_check.cpp applies the HOST RESTATEMENT of the update -- the plan build_layout keeps, the argument checks,
the per-instance records, re-padding, refit and cull factors, the very functions the kernels are made of -- to build_layout(base).
The bar: the resulting pair, instance and triangle records are byte-equal to build_layout(scenes.refit_instances(base, moved)), i.e.
to what a full upload of the refit scene makes.

One exception is measured and pinned here rather than hidden.  With leaf subdivision at max_leaf_tris = 2 (the library's default for
small scenes), a scene of at most 2 046 triangle slots orders its slots by the surface area of their leaf's PADDED box
(scene_layout.h, tiny-scene mode), and the padding depends on the instance matrices: a full upload of the moved scene may swap two
leaves of equal size (seen: moving_instances and the one-instance Cornell box, two leaf references swapped).  The update re-pads the
boxes but keeps the slot order, which no result depends on.  For that leaf size the pair records are therefore compared with every
triangle-leaf reference resolved to the scene triangles it names; where the triangle records do agree, the bytes must too.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import instance_update_cases as cases
from conftest import ROOT, bits
from polaris_amd import ctypes_api as T
from polaris_amd import scenes

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "instance_update_check.cpp")
LIB = os.path.join(BUILD, "libinstance_update_check.so")
CAP = 1 << 22
TRI_RECORD = np.dtype([("v0", "<f4", 3), ("rank", "<u4"), ("e1", "<f4", 3), ("orig", "<u4"), ("e2", "<f4", 3), ("word", "<u4")])
E_BAD_ARGUMENT, E_BAD_SCENE, E_UNSUPPORTED = 2, 5, 6


@pytest.fixture(scope="module")
def tool():
    os.makedirs(BUILD, exist_ok=True)
    csrc = os.path.join(ROOT, "polaris_amd", "csrc")
    deps = [SRC, os.path.join(csrc, "scene_layout.h"), os.path.join(csrc, "instance_update.h"), os.path.join(ROOT, "include", "polaris_hip.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, SRC, "-o", LIB])
    return C.CDLL(LIB)


class Records:
    def __init__(self):
        self.bufs = [np.zeros(CAP, np.uint8) for _ in range(3)]
        self.counts = np.zeros(3, np.uint32)
        self.err = C.create_string_buffer(512)

    def args(self):
        return [C.c_void_p(b.ctypes.data) for b in self.bufs] + [C.c_size_t(CAP), C.c_void_p(self.counts.ctypes.data)]

    def take(self):
        p, i, t = self.bufs
        return (p[:int(self.counts[0]) * 64].view(T.PAIR_RECORD).copy(), i[:int(self.counts[1]) * 64].view(T.INST_RECORD).copy(),
                t[:int(self.counts[2]) * 48].view(TRI_RECORD).copy())


def layout(tool, sc, max_leaf):
    """(pairs, insts, tris) of build_layout(sc)."""
    r, view = Records(), T.scene_view(sc)
    rc = tool.iu_layout(C.byref(view), max_leaf, *r.args(), r.err, C.c_size_t(512))
    assert rc == 0, r.err.value.decode()
    return r.take()


def update(tool, base, max_leaf, u, option_on=True):
    """(records, status, message, plan sizes): build_layout(base) with the restated update `u` applied."""
    r, view = Records(), T.scene_view(base)
    status, sizes = C.c_int(0), np.zeros(5, np.uint32)
    rc = tool.iu_update(C.byref(view), max_leaf, int(option_on), C.byref(u) if u is not None else None, *r.args(), C.byref(status),
                        C.c_void_p(sizes.ctypes.data), r.err, C.c_size_t(512))
    assert rc == 0, r.err.value.decode()
    return r.take(), status.value, r.err.value.decode(), sizes


def resolved(pairs, tris):
    """The pair records with every triangle-leaf reference replaced by the scene triangles it names."""
    out = []
    for p in pairs:
        refs = []
        for ref in (int(p["ref0"]), int(p["ref1"])):
            code = ~ref & 0xFFFFFFFF
            if ref < 0 and code & 15:
                ref = tuple(int(o) & 0xFFFFFF for o in tris["orig"][code >> 4:(code >> 4) + (code & 15)])
            refs.append(ref)
        out.append((p["lo0"].tobytes(), p["hi0"].tobytes(), p["cull0"].tobytes(), p["lo1"].tobytes(), p["hi1"].tobytes(), p["cull1"].tobytes(), *refs))
    return out


# ---- 1. the restated update against a full layout of the refit scene -----------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [0, 2, 4])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_restated_update_equals_layout_of_refit_scene(tool, name, max_leaf):
    base, moved, refit = cases.case(name)
    want = layout(tool, refit, max_leaf)
    u, keep = T.instance_update(*scenes.instance_update_args(moved))
    got, status, msg, sizes = update(tool, base, max_leaf, u)
    assert status == 0, msg
    assert sizes[0] == 2 * len(base.mesh_instances) - 1 and sizes[3] > 0
    before = layout(tool, base, max_leaf)
    assert not np.array_equal(got[1], before[1]), "the case moves nothing"
    assert got[1].tobytes() == want[1].tobytes(), "instance records"
    if max_leaf != 2 or got[2].tobytes() == want[2].tobytes():
        assert got[2].tobytes() == want[2].tobytes(), "triangle records"
        assert got[0].tobytes() == want[0].tobytes(), "pair records"
    else:   # the slot order of a tiny scene followed the padding (module docstring)
        assert len(got[2]) <= 2046 and sorted(got[2]["orig"]) == sorted(want[2]["orig"])
        assert resolved(got[0], got[2]) == resolved(want[0], want[2]), "pair records, leaf references resolved"
    if name == "transformed-returned":   # cull factors flipped in both directions
        inf = np.isinf
        a, b = np.concatenate([before[0]["cull0"], before[0]["cull1"]]), np.concatenate([got[0]["cull0"], got[0]["cull1"]])
        assert (inf(a) & ~inf(b)).any() and (~inf(a) & inf(b)).any()
    if name == "one-instance":
        assert sizes[0] == 1 and sizes[1] == 1


def test_subdivision_padding_follows_the_move(tool):
    """The boxes leaf subdivision added are re-padded: the turning block's padding grows with the turn (the room's corners move
    away from the block's axes), and the records still equal the full layout's."""
    base, moved, refit = cases.case("moving-0-8")
    u, keep = T.instance_update(*scenes.instance_update_args(moved))
    got, status, _, sizes = update(tool, base, 2, u)
    assert status == 0 and sizes[4] > 0
    before, want = layout(tool, base, 2), layout(tool, refit, 2)
    mesh_level = np.array([a.tobytes() != b.tobytes() for a, b in zip(before[0], want[0])])
    assert mesh_level.sum() > 2          # more than the two top-level records differ between the two full layouts ...
    assert resolved(got[0], got[2]) == resolved(want[0], want[2])   # ... and the update follows


# ---- 2. refit_instances against a plain loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moving-0-8", "transformed-returned", "swarm-150", "one-instance"])
def test_refit_instances_equals_a_plain_bottom_up_loop(name):
    base, moved, refit = cases.case(name)
    boxes = scenes.instance_boxes(moved)
    nodes = base.bvh_nodes.copy()

    def fit(i):
        n = nodes[i]
        if n["ldata"] <= 0:
            inst = -int(n["ldata"])
            nodes["min"][i], nodes["max"][i] = boxes[inst, :3], boxes[inst, 3:]
            return
        l, r = int(n["ldata"]), int(n["rdata"])
        fit(l)
        fit(r)
        for k in range(3):
            a, b = nodes["min"][l][k], nodes["min"][r][k]
            nodes["min"][i][k] = b if b < a else a
            a, b = nodes["max"][l][k], nodes["max"][r][k]
            nodes["max"][i][k] = b if b > a else a

    fit(0)
    assert refit.bvh_nodes.tobytes() == nodes.tobytes()
    assert refit.mesh_instances["inv_transform"].tobytes() == moved.mesh_instances["inv_transform"].tobytes()
    assert refit.emissives.tobytes() == moved.emissives.tobytes()
    assert refit.mesh_instances["bvh_root"].tobytes() == base.mesh_instances["bvh_root"].tobytes()
    # fmin / fmax agree wherever no +0 meets a -0
    top = scenes._top_level_nodes(refit)[0]
    inner = top[refit.bvh_nodes["ldata"][top] > 0]
    l, r = refit.bvh_nodes["ldata"][inner], refit.bvh_nodes["rdata"][inner]
    assert np.array_equal(refit.bvh_nodes["min"][inner], np.fmin(refit.bvh_nodes["min"][l], refit.bvh_nodes["min"][r]))
    assert np.array_equal(refit.bvh_nodes["max"][inner], np.fmax(refit.bvh_nodes["max"][l], refit.bvh_nodes["max"][r]))


# ---- 3. a refit changes no hit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moving-0-1", "transformed-returned", "swarm-17", "swarm-150"])
def test_oracle_trace_of_refit_scene_equals_the_moved_scene_compiled_afresh(oracle, name):
    """Three of the four differ from the freshly compiled scene in top-level topology.  Not here: moving-0-8.  Its blocks stand ON the
    floor of another instance, so rays that reach the shared plane at a block's foot have two exactly tied hits; the reference's
    "first tested wins" follows the top-level order there, which a refit keeps and a fresh compile changes (one pixel of 48 x 36 at
    step 8 -- the topology dependence is the reference's, tests/test_gpu_ties.py).  The scenes here have no coplanar instances."""
    from oracle import pybind as ob

    _, moved, refit = cases.case(name)
    W, H, spp, bounces = 48, 36, 2, 3
    seeds = scenes.make_seeds(spp, bounces, base=11)
    want, ws, _ = oracle.trace(moved, ob.make_request(W, H, spp=spp, bounces=bounces), seeds)
    got, gs, _ = oracle.trace(refit, ob.make_request(W, H, spp=spp, bounces=bounces), seeds)
    assert np.array_equal(bits(got), bits(want))
    assert list(gs.rays_per_bounce) == list(ws.rays_per_bounce) and list(gs.occl_per_bounce) == list(ws.occl_per_bounce)
    assert np.abs(want[..., :3]).sum() > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def _refusals(base, moved):
    inv, boxes, ems = scenes.instance_update_args(moved)
    NI = len(inv)

    def edit(arr, fn):
        a = arr.copy()
        fn(a)
        return a

    def nan_entry(a): a[1, 5] = np.nan
    def big_entry(a): a[NI - 1, 12] = np.float32(2.0 ** 30 * 1.0001)
    def inf_box(a): a[0, 4] = np.inf
    def flipped_box(a): a[1, 0], a[1, 3] = a[1, 3] + 1.0, a[1, 0]
    def other_triangle(a): a["tri_index"][0] += 1
    def other_type(a): a["type"][0] = T.EMISSIVE_ENVIRONMENT
    def other_node(a): a["mat_node_index"][0] += 1

    def with_size(u, size):
        u.struct_size = size
        return u

    def with_null(u, field):
        setattr(u, field, None)
        return u

    mk = T.instance_update
    yield "option off", E_UNSUPPORTED, mk(inv, boxes, ems), False
    yield "struct_size", E_BAD_ARGUMENT, (lambda uk: (with_size(uk[0], uk[0].struct_size + 8), uk[1]))(mk(inv, boxes, ems)), True
    yield "instance count", E_BAD_ARGUMENT, mk(inv[:-1], boxes[:-1], ems), True
    yield "null matrices", E_BAD_ARGUMENT, (lambda uk: (with_null(uk[0], "inv_transforms"), uk[1]))(mk(inv, boxes, ems)), True
    yield "null boxes", E_BAD_ARGUMENT, (lambda uk: (with_null(uk[0], "instance_boxes"), uk[1]))(mk(inv, boxes, ems)), True
    yield "NaN matrix entry", E_BAD_SCENE, mk(edit(inv, nan_entry), boxes, ems), True
    yield "matrix entry beyond 2^30", E_BAD_SCENE, mk(edit(inv, big_entry), boxes, ems), True
    yield "infinite box", E_BAD_SCENE, mk(inv, edit(boxes, inf_box), ems), True
    yield "box min > max", E_BAD_SCENE, mk(inv, edit(boxes, flipped_box), ems), True
    yield "emissive count", E_BAD_ARGUMENT, mk(inv, boxes, np.concatenate([ems, ems[:1]])), True
    yield "emissive triangle", E_BAD_ARGUMENT, mk(inv, boxes, edit(ems, other_triangle)), True
    yield "emissive type", E_BAD_ARGUMENT, mk(inv, boxes, edit(ems, other_type)), True
    yield "emissive material node", E_BAD_ARGUMENT, mk(inv, boxes, edit(ems, other_node)), True


def test_refusals_return_their_status_and_change_nothing(tool):
    """Each refusal returns its status with a message, and the restatement has touched no record when it refuses (the records it
    hands back are build_layout(base)'s).  The tool rebuilds the layout for every call, so it holds no state a refusal could spoil:
    that a refused call leaves a TRACER as it was is shown on the device (tests/test_gpu_instance_update.py, refusals)."""
    base, moved, refit = cases.case("transformed-returned")
    untouched = layout(tool, base, 2)
    want = layout(tool, refit, 2)
    for what, status, (u, keep), option_on in _refusals(base, moved):
        got, st, msg, _ = update(tool, base, 2, u, option_on)
        assert st == status and msg, (what, st, msg)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, untouched)), what
    got, st, msg, _ = update(tool, base, 2, None)
    assert st == E_BAD_ARGUMENT
    good, keep = T.instance_update(*scenes.instance_update_args(moved))          # (the same arguments unedited are accepted)
    got, st, msg, _ = update(tool, base, 2, good)
    assert st == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
