"""CPU test of the mask of shading classes that can end in an emitter (polaris_amd/csrc/scene_layout.h, emitting_classes).

The shade kernels retire a ray that Russian roulette rejects without shading its hit when the hit's class has a CLEAR bit in that
mask (kernels.h, shade_fate), so a bit may be set for a class that never emits but must never be clear for one that can.
tests/tools/class_mask_check.cpp runs shading_classes() and emitting_classes() on a bare material node table.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from polaris_amd import ctypes_api as T
from polaris_amd.scenes import MaterialTable

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "class_mask_check.cpp")
LIB = os.path.join(BUILD, "libclass_mask_check.so")


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "scene_layout.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    return C.CDLL(LIB)


def classes_and_mask(lib, mt):
    nodes = np.ascontiguousarray(np.array(mt.nodes, dtype=T.MATERIAL_NODE))
    cls = np.zeros(len(nodes), np.uint8)
    mask = C.c_uint32(0)
    assert lib.class_mask_check(C.c_void_p(nodes.ctypes.data), C.c_uint32(len(nodes)), C.c_void_p(cls.ctypes.data), C.byref(mask)) == 0
    assert cls.min() >= 1 and cls.max() <= 15
    return [int(c) for c in cls], mask.value


def bit(mask, c):
    return (mask >> c) & 1


def test_emissive_only(lib):
    mt = MaterialTable()
    e = mt.emissive()
    cls, mask = classes_and_mask(lib, mt)
    assert mask == 1 << cls[e]


def test_mix_with_an_emissive_child_and_a_bump_mapped_emissive(lib):
    mt = MaterialTable()
    e, d, c = mt.emissive(), mt.diffuse(), mt.conductor()
    m = mt.mix(d, e, 0.5)          # emissive on the right
    mm = mt.mix_map(e, c, 0)       # ... on the left of a textured mix
    b = mt.bump_map(e, 0)
    n = mt.normal_map(m, 0)        # two operators above the leaf
    plain = mt.mix(d, c, 0.5)
    disp = mt.disperse(mt.dielectric(), (1.5, 1.51, 1.52), (1, 1, 1))
    cls, mask = classes_and_mask(lib, mt)
    assert len(set(cls)) == len(cls)       # (ten nodes, ten reach sets: every class below is one set)
    for i in (e, m, mm, b, n):
        assert bit(mask, cls[i]), i
    for i in (d, c, plain, disp):
        assert not bit(mask, cls[i]), i


def test_an_invalid_child_sets_nothing(lib):
    mt = MaterialTable()
    d = mt.diffuse()
    bad_leaf = mt._node(T.BXDF_INVALID)
    dangling = mt.mix(d, 99, 0.5)                  # right child out of range
    over_bad = mt.bump_map(bad_leaf, 0)
    unknown_op = mt._node(10009, left_child=0)
    cls, mask = classes_and_mask(lib, mt)
    assert mask == 0
    e = mt.emissive()
    both = mt.mix(e, 99, 0.5)                      # one child ends the path, the other is an emitter
    cls, mask = classes_and_mask(lib, mt)
    assert bit(mask, cls[e]) and bit(mask, cls[both])
    assert not any(bit(mask, cls[i]) for i in (d, bad_leaf, dangling, over_bad, unknown_op))


def test_a_cycle_is_walked_like_any_other_edge(lib):
    """mix(bump(-> the mix itself), emissive): the device walk from the BUMP node reaches the emitter through the cycle (select_material
    follows up to 64 edges), although the reach set of the bump node, closed while the mix was still on the walk, lacks it."""
    mt = MaterialTable()
    e = mt.emissive()
    bump = mt.bump_map(0, 0)       # child patched below
    m = mt.mix(bump, e, 0.5)
    mt.nodes[bump]["left_child"] = m
    lonely = mt.bump_map(0, 0)
    mt.nodes[lonely]["left_child"] = lonely   # a cycle that reaches nothing
    cls, mask = classes_and_mask(lib, mt)
    assert bit(mask, cls[e]) and bit(mask, cls[m]) and bit(mask, cls[bump])
    assert not bit(mask, cls[lonely]) or cls[lonely] in (cls[e], cls[m], cls[bump])


def test_more_reach_sets_than_classes_share_class_15(lib):
    mt = MaterialTable()
    leaves = [mt.diffuse(), mt.conductor(), mt.rough_conductor(), mt.dielectric(), mt.rough_dielectric()]
    roots = []
    for a in range(5):             # 10 two-leaf mixes + 10 bump-mapped ones + 5 leaves: 25 reach sets without an emitter
        for b in range(a + 1, 5):
            roots.append(mt.mix(leaves[a], leaves[b], 0.5))
            roots.append(mt.bump_map(roots[-1], 0))
    cls, mask = classes_and_mask(lib, mt)
    assert len(set(cls)) == 15 and cls.count(15) > 1
    assert mask == 0                                # no emitter anywhere: class 15 stays clear too
    e = mt.emissive()
    # an emitter under a root whose reach set sorts last: it lands in the shared class
    top = mt.disperse(mt.bump_map(mt.mix(leaves[4], e, 0.5), 0), (1.5, 1.5, 1.5), (1, 1, 1))
    cls, mask = classes_and_mask(lib, mt)
    assert cls[top] == 15 and bit(mask, 15)
    assert bit(mask, cls[e])
    for i in range(len(cls)):                       # below 15 a class is one reach set: its bit is exact
        if cls[i] < 15:
            reaches = i == e or (int(mt.nodes[i]["type"]) >= T.OP_MIX and _reaches(mt, i, e))
            assert bit(mask, cls[i]) == int(reaches), i


def _reaches(mt, i, target, depth=0):
    if i == target:
        return True
    n = mt.nodes[i]
    t = int(n["type"])
    if t < T.OP_MIX or depth > 8:
        return False
    kids = [int(n["left_child"])] + ([int(n["right_child"])] if t in (T.OP_MIX, T.OP_MIX_MAP) else [])
    return any(0 <= k < len(mt.nodes) and _reaches(mt, k, target, depth + 1) for k in kids)
