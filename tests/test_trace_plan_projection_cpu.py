"""CPU test of what a projection (TraceScene::projection, polaris_amd/csrc/trace_plan.h; polaris_hip_set_projection) changes in the
plan of a Trace, over the option grid of tests/test_trace_plan_lens_cpu.py: it plans exactly as the lens does -- the generator always
writes the origins, bounce 0's closest-hit rays are RayKind::Closest, traced by the kernels the lens' plan names, so neither the
shared-origin camera launch nor the camera packet kernel is used -- and every other field of the plan is the projection-off plan's.
With the projection off the plan is what it was: test_trace_plan_cpu.py, test_trace_plan_lens_cpu.py and
test_trace_plan_shutter_cpu.py run unchanged.
"""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from test_trace_plan_cpu import CAMERA, CLOSEST, IN_FIELDS, MAX_BOUNCES
from test_trace_plan_lens_cpu import GRID, grid

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "trace_plan_projection_check.cpp")
LIB = os.path.join(BUILD, "libtrace_plan_projection_check.so")

CAMERA_FLAGS = ["lens", "shutter", "projection"]
PROJECTION_IN = [k for k in IN_FIELDS if k not in ("clamp", "available")]
PROJECTION_IN[PROJECTION_IN.index("num_cus") + 1:PROJECTION_IN.index("num_cus") + 1] = CAMERA_FLAGS
SCALARS = ["K", "n_batches", "n_pipes", "wants_memory_clamp", "exact", "staged", "moments", "prefilter", "hit12", "o12", "generate_writes_origins",
           "primary", "scene_lens", "scene_shutter", "scene_projection"]
LIKE_THE_LENS = ("generate_writes_origins", "primary", "isect")


class PlanIn(C.Structure):
    _fields_ = [(name, C.c_int64) for name in PROJECTION_IN]


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
    so.trace_plan_projection_check.restype = None
    return so


def plan(lib, **kw):
    fields = {k: IN_FIELDS[k] for k in PROJECTION_IN if k not in CAMERA_FLAGS}
    fields.update({k: 0 for k in CAMERA_FLAGS})
    unknown = set(kw) - set(fields)
    assert not unknown, unknown
    out = PlanOut()
    lib.trace_plan_projection_check(C.byref(PlanIn(**dict(fields, **kw))), C.byref(out))
    return {name: (list(getattr(out, name)) if name in ("isect", "occl", "shade", "grids") else getattr(out, name)) for name, _ in PlanOut._fields_}


def test_a_projection_plans_as_the_lens_does_and_changes_nothing_else(lib):
    cases = 0
    for kw in grid():
        off, lens, on = plan(lib, **kw), plan(lib, lens=1, **kw), plan(lib, projection=1, **kw)
        assert (off["scene_projection"], off["primary"]) == (0, CAMERA), kw
        assert (on["scene_lens"], on["scene_shutter"], on["scene_projection"]) == (0, 0, 1), kw
        assert on["generate_writes_origins"] == 1 and on["primary"] == CLOSEST, kw
        for name in LIKE_THE_LENS:                                  # projection on = lens on
            assert on[name] == lens[name], (name, kw)
        for name in on:                                             # every other field: the projection-off plan's
            if name not in LIKE_THE_LENS + ("scene_projection",):
                assert on[name] == off[name], (name, kw)
        cases += 1
    assert cases == 2304
    n = 1
    for values in GRID.values():
        n *= len(values)
    assert n == 2304


def test_the_headline_plan_keeps_its_batches_and_grids_under_a_projection(lib):
    head = dict(Npad=1024 * 1024, spp=32, tiny=1, resident_closest=2, resident_any=2, scene_packet_primary=0)
    off, on = plan(lib, **head), plan(lib, projection=1, **head)
    assert (off["K"], off["n_batches"], off["n_pipes"]) == (on["K"], on["n_batches"], on["n_pipes"]) == (16, 2, 2)
    assert off["grids"] == on["grids"] and off["shade"] == on["shade"] and off["occl"] == on["occl"]
    assert on["primary"] == CLOSEST and off["generate_writes_origins"] == 0 and on["generate_writes_origins"] == 1
