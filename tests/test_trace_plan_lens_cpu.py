"""CPU test of what the thin lens (TraceScene::lens, polaris_amd/csrc/trace_plan.h) changes in the plan of a Trace, over the option grid
of tests/test_trace_plan_cpu.py: the generator always writes the origins, bounce 0's closest-hit rays are planned as RayKind::Closest
(the packet kernel exactly where the upload resolved packet_primary, else k_trace or k_intersect by `traversal`), and every other
field of the plan is the lens-off plan's.  With the lens off the plan is what it was: test_trace_plan_cpu.py runs unchanged.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from conftest import ROOT
from test_trace_plan_cpu import CAMERA, CLOSEST, IN_FIELDS, MAX_BOUNCES, PACKET, PERSISTENT, PLAIN

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "trace_plan_lens_check.cpp")
LIB = os.path.join(BUILD, "libtrace_plan_lens_check.so")

LENS_IN = [k for k in IN_FIELDS if k not in ("clamp", "available")]
LENS_IN.insert(LENS_IN.index("num_cus") + 1, "lens")
SCALARS = ["K", "n_batches", "n_pipes", "wants_memory_clamp", "exact", "staged", "moments", "prefilter", "hit12", "o12", "generate_writes_origins",
           "primary", "scene_lens"]
CHANGED = ("generate_writes_origins", "primary", "scene_lens")


class PlanIn(C.Structure):
    _fields_ = [(name, C.c_int64) for name in LENS_IN]


class PlanOut(C.Structure):
    _fields_ = [(name, C.c_int64) for name in SCALARS] + [(name, C.c_int64 * MAX_BOUNCES) for name in ("isect", "occl", "shade")] + [("grids", C.c_int64 * 3)]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "trace_plan.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    so.trace_plan_lens_check.restype = None
    return so


def plan(lib, **kw):
    fields = {k: IN_FIELDS[k] for k in LENS_IN if k != "lens"}
    fields["lens"] = 0
    unknown = set(kw) - set(fields)
    assert not unknown, unknown
    out = PlanOut()
    lib.trace_plan_lens_check(C.byref(PlanIn(**dict(fields, **kw))), C.byref(out))
    return {name: (list(getattr(out, name)) if name in ("isect", "occl", "shade", "grids") else getattr(out, name)) for name, _ in PlanOut._fields_}


# the options the existing plan test varies where a Trace chooses kernels, batches and grids
GRID = dict(scene_packet_primary=(0, 1), packet_primary=(-1, 0, 1), traversal=(0, 1), packet_shadow=(0, 2), exact=(0, 1), bounces=(0, 1, 4),
            shade_wave=(0, 1), o12=(0, 1), tiny=(0, 1), samples_per_batch=(0, 3))


def grid():
    keys = list(GRID)
    for values in itertools.product(*(GRID[k] for k in keys)):
        yield dict(zip(keys, values))


def test_the_lens_changes_the_origins_and_the_kind_of_bounce_0_and_nothing_else(lib):
    cases = 0
    for kw in grid():
        off, on = plan(lib, lens=0, **kw), plan(lib, lens=1, **kw)
        B = kw["bounces"]
        assert (off["scene_lens"], on["scene_lens"]) == (0, 1)
        assert on["generate_writes_origins"] == 1, kw                       # every kernel that traces lens rays reads the origin stream
        assert (off["primary"], on["primary"]) == (CAMERA, CLOSEST), kw
        if B:
            first = PACKET if kw["scene_packet_primary"] else (PERSISTENT if kw["traversal"] else PLAIN)
            assert on["isect"][0] == first, kw
            assert on["isect"][1:B] == [PERSISTENT if kw["traversal"] else PLAIN] * (B - 1), kw
        for name in off:
            if name not in CHANGED:
                assert off[name] == on[name], (name, kw)
        cases += 1
    assert cases == 2 * 3 * 2 * 2 * 2 * 3 * 2 * 2 * 2 * 2


def test_lens_off_writes_origins_only_where_a_kernel_reads_them(lib):
    """(What test_trace_plan_cpu.py pins, through this tap: the lens-off column of the comparison above is the plan as it was.)"""
    assert plan(lib)["generate_writes_origins"] == 0
    assert plan(lib, scene_packet_primary=0, traversal=0)["generate_writes_origins"] == 1
    assert plan(lib, lens=1)["generate_writes_origins"] == 1
    assert plan(lib, lens=1, scene_packet_primary=0)["generate_writes_origins"] == 1
    assert plan(lib, lens=1, bounces=0)["generate_writes_origins"] == 1


def test_the_headline_plan_keeps_its_batches_and_grids_under_a_lens(lib):
    head = dict(Npad=1024 * 1024, spp=32, tiny=1, resident_closest=2, resident_any=2, scene_packet_primary=0)
    off, on = plan(lib, **head), plan(lib, lens=1, **head)
    assert (off["K"], off["n_batches"], off["n_pipes"]) == (on["K"], on["n_batches"], on["n_pipes"]) == (16, 2, 2)
    assert off["grids"] == on["grids"] and off["shade"] == on["shade"]
    assert on["isect"][:4] == [PERSISTENT] * 4 and on["primary"] == CLOSEST
