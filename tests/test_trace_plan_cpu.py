"""CPU test of what a Trace decides (polaris_amd/csrc/trace_plan.h): the batch size with its memory clamp and its halving after a
failed allocation, the batches and pipelines, the shade kernel of every bounce, the grids of the persistent launches and the
traversal kernel of a ray set.

tests/tools/trace_plan_check.cpp hands plain numbers to the header's functions.  Every expectation below is worked out by hand
from the rules (the arithmetic stands beside it); none is read back from the library.
"""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "trace_plan_check.cpp")
LIB = os.path.join(BUILD, "libtrace_plan_check.so")

MAX_BOUNCES = 32
PACKET, PERSISTENT, PLAIN = 0, 1, 2          # Traversal
CAMERA, CLOSEST, ANY_HIT = 0, 1, 2           # RayKind
FIRST, SORT, PLAIN_SHADE, WAVE = 0, 1, 2, 3  # ShadeKernel

# the defaults: the options as a new handle has them, a 256-CU device, a scene whose k_trace variants fit six to a CU, whose tables fit
# LDS, with one emitting class of several, and whose upload resolved packet_primary to on
IN_FIELDS = dict(samples_per_batch=0, exact=0, overlap=4, packet_shadow=0, packet_primary=-1, traversal=1, trace_wgs_per_cu=0, trace_grid=0,
                 stage_lds=1, shade_wave=1, shade_wgs_per_cu=4, shade_wave_from=-1, shade_prefilter=1, shade_sort=-1, hit12=1, o12=1,
                 tiny=0, resident_closest=6, resident_any=6, tables_fit_lds=1, emit_classes=0x0002, tri_bits=20, scene_packet_primary=1, num_cus=256,
                 moments=0, spp=4, bounces=4, min_rr=2, Npad=64 * 48,
                 clamp=0, available=0)
OUT_SCALARS = ["K", "n_batches", "n_pipes", "wants_memory_clamp", "exact", "staged", "moments", "prefilter", "hit12", "o12", "generate_writes_origins"]


class PlanIn(C.Structure):
    _fields_ = [(name, C.c_int64) for name in IN_FIELDS]


class PlanOut(C.Structure):
    _fields_ = [(name, C.c_int64) for name in OUT_SCALARS] + [(name, C.c_int64 * MAX_BOUNCES) for name in ("isect", "occl", "shade")]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "trace_plan.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    for name in ("trace_plan_shrunk", "trace_plan_bytes_needed", "trace_plan_slot_bytes", "trace_plan_batch_traversal", "trace_plan_probe_traversal",
                 "trace_plan_tap_traversal", "trace_plan_probe_grid", "trace_plan_tables_staged"):
        getattr(so, name).restype = C.c_int64
    so.trace_plan_timer.restype = C.c_char_p
    so.trace_plan_check.restype = None
    so.trace_plan_grids.restype = None
    return so


def make_in(**kw):
    unknown = set(kw) - set(IN_FIELDS)
    assert not unknown, unknown
    return PlanIn(**dict(IN_FIELDS, **kw))


def plan(lib, shrinks=None, **kw):
    out = PlanOut()
    if shrinks is None:
        lib.trace_plan_check(C.byref(make_in(**kw)), C.byref(out))
        return out
    taken = lib.trace_plan_shrunk(C.byref(make_in(**kw)), C.c_int64(shrinks), C.byref(out))
    return out, taken


def batches(p):
    return (p.K, p.n_batches, p.n_pipes)


def column(p, what, bounces):
    col = list(getattr(p, what))
    assert col[bounces:] == [-1] * (MAX_BOUNCES - bounces)   # nothing is planned past the request's bounces
    return col[:bounces]


def grids(lib, wgs, **kw):
    g = (C.c_int64 * 3)()
    lib.trace_plan_grids(C.byref(make_in(**kw)), C.c_int64(wgs), g)
    return list(g)


MI = 1 << 20
HEADLINE = 1024 * 1024   # path slots of a 1024 x 1024 frame: 4096 chunks of 256


# ---- the batch size

def test_automatic_batch_size(lib):
    """K = min(32 Mi / Npad, (spp + 1) / 2), at least 1; pipelines = min(overlap, batches)."""
    assert batches(plan(lib, Npad=HEADLINE, spp=32)) == (16, 2, 2)     # min(32, 16): two batches of 16
    assert batches(plan(lib, Npad=HEADLINE, spp=256)) == (32, 8, 4)    # min(32, 128): the path budget binds; 8 batches on 4 pipelines
    assert batches(plan(lib, Npad=64 * 48, spp=2)) == (1, 2, 2)        # min(10922, 1)
    assert batches(plan(lib, Npad=16 * MI, spp=32)) == (2, 16, 4)      # the largest block: 32 Mi / 16 Mi = 2
    assert batches(plan(lib, Npad=3 * MI, spp=64)) == (10, 7, 4)       # 32 / 3 rounds down to 10; ceil(64 / 10) = 7
    assert batches(plan(lib, Npad=HEADLINE, spp=5)) == (3, 2, 2)       # (5 + 1) / 2 = 3: batches of 3 and 2
    assert batches(plan(lib, Npad=HEADLINE, spp=256, overlap=1)) == (32, 8, 1)
    assert batches(plan(lib, Npad=HEADLINE, spp=256, overlap=8)) == (32, 8, 8)


def test_no_samples_and_one_sample(lib):
    assert batches(plan(lib, spp=0)) == (1, 0, 1)    # nothing to trace: no batch, and still one pipeline (the main stream)
    assert batches(plan(lib, spp=1)) == (1, 1, 1)    # (1 + 1) / 2 = 1
    assert batches(plan(lib, spp=0, samples_per_batch=8)) == (1, 0, 1)   # min(8, max(spp, 1))


def test_exact_mode_traces_one_sample_at_a_time_on_one_pipeline(lib):
    p = plan(lib, Npad=HEADLINE, spp=32, exact=1)
    assert batches(p) == (1, 32, 1) and p.exact == 1
    assert batches(plan(lib, Npad=HEADLINE, spp=32, exact=1, samples_per_batch=8)) == (1, 32, 1)


def test_a_chosen_batch_size_is_capped_at_4096_and_at_the_sample_count(lib):
    assert batches(plan(lib, spp=10000, samples_per_batch=5000)) == (4096, 3, 3)   # ceil(10000 / 4096) = 3
    assert batches(plan(lib, spp=10000, samples_per_batch=4096)) == (4096, 3, 3)
    assert batches(plan(lib, spp=5, samples_per_batch=9)) == (5, 1, 1)
    assert batches(plan(lib, spp=7, samples_per_batch=3)) == (3, 3, 3)             # 3 + 3 + 1
    assert batches(plan(lib, Npad=HEADLINE, spp=256, samples_per_batch=64)) == (64, 4, 4)   # (not held to the 32 Mi path budget)


# ---- the memory clamp and the halving after a failed allocation

def test_slot_bytes(lib):
    assert lib.trace_plan_slot_bytes(C.c_int64(4)) == 144 + 17 * 4 == 212
    assert lib.trace_plan_slot_bytes(C.c_int64(1)) == 161
    assert lib.trace_plan_slot_bytes(C.c_int64(0)) == 161    # a Trace without bounces still holds one NEE array
    assert lib.trace_plan_slot_bytes(C.c_int64(32)) == 688


def test_memory_clamp_where_halving_brings_more_batches_into_flight(lib):
    """1024 x 1024, 32 spp, 4 bounces, overlap 4, free + held = 4 000 000 000 B: 212 B a slot, budget 3 600 000 000 B.  K = 16 runs 2
    batches at once, K = 8 runs 4: the same 7 113 539 584 B.  K = 4 still runs 4: 3 556 769 792 B fits."""
    case = dict(Npad=HEADLINE, spp=32, bounces=4, overlap=4)
    need = lambda k: lib.trace_plan_bytes_needed(C.byref(make_in(**case)), C.c_int64(k))
    assert need(16) == 16 * HEADLINE * 212 * 2 == 7113539584
    assert need(8) == 8 * HEADLINE * 212 * 4 == 7113539584
    assert need(4) == 4 * HEADLINE * 212 * 4 == 3556769792
    unclamped = plan(lib, **case)
    assert batches(unclamped) == (16, 2, 2) and unclamped.wants_memory_clamp == 1
    assert batches(plan(lib, clamp=1, available=4000000000, **case)) == (4, 8, 4)
    # nine tenths of what is available: 3 952 000 000 B give 3 556 800 000 (K = 4 fits by 30 208 B), 3 951 900 000 B do not
    assert batches(plan(lib, clamp=1, available=3952000000, **case)) == (4, 8, 4)
    assert batches(plan(lib, clamp=1, available=3951900000, **case)) == (2, 16, 4)
    assert batches(plan(lib, clamp=1, available=288 * 10**9, **case)) == (16, 2, 2)    # ample: untouched
    assert batches(plan(lib, clamp=1, available=7904000000, **case)) == (16, 2, 2)     # budget 7 113 600 000 >= the need
    assert batches(plan(lib, clamp=1, available=1, **case)) == (1, 32, 4)              # nothing fits: it stops at 1
    assert batches(plan(lib, clamp=1, available=4000000000, **dict(case, overlap=1))) == (16, 2, 1)  # one batch in flight: 16 x 1 Mi x 212 = 3 556 769 792 fits
    assert batches(plan(lib, clamp=1, available=2000000000, **dict(case, overlap=1))) == (8, 4, 1)   # budget 1 800 000 000 >= 1 778 384 896


def test_a_chosen_batch_size_and_exact_mode_are_never_clamped(lib):
    case = dict(Npad=HEADLINE, spp=32, bounces=4, clamp=1, available=1000)
    p = plan(lib, samples_per_batch=16, **case)
    assert batches(p) == (16, 2, 2) and p.wants_memory_clamp == 0
    p = plan(lib, exact=1, **case)
    assert batches(p) == (1, 32, 1) and p.wants_memory_clamp == 0
    assert plan(lib, Npad=64 * 48, spp=2).wants_memory_clamp == 0    # K = 1 has nothing to give


def test_failed_allocations_halve_the_batch_down_to_one(lib):
    case = dict(Npad=HEADLINE, spp=32, bounces=4)
    for shrinks, want in [(0, (16, 2, 2)), (1, (8, 4, 4)), (2, (4, 8, 4)), (3, (2, 16, 4)), (4, (1, 32, 4))]:
        p, taken = plan(lib, shrinks=shrinks, **case)
        assert (batches(p), taken) == (want, shrinks)
    p, taken = plan(lib, shrinks=10, **case)
    assert batches(p) == (1, 32, 4) and taken == 4          # at K = 1 the failure is final
    p, taken = plan(lib, shrinks=10, Npad=HEADLINE, spp=14)    # odd sizes round up: 7 -> 4 -> 2 -> 1
    assert batches(p) == (1, 14, 4) and taken == 3
    p, taken = plan(lib, shrinks=1, Npad=HEADLINE, spp=14)
    assert batches(p) == (4, 4, 4)
    p, taken = plan(lib, shrinks=3, samples_per_batch=16, **case)   # the caller's choice: reported, not retried
    assert batches(p) == (16, 2, 2) and taken == 0
    p, taken = plan(lib, shrinks=3, exact=1, **case)
    assert batches(p) == (1, 32, 1) and taken == 0
    p, taken = plan(lib, shrinks=2, clamp=1, available=4000000000, **case)   # after the clamp's 4: 2, 1
    assert batches(p) == (1, 32, 4) and taken == 2


# ---- the grids

BIG = 65536   # chunks: more than any grid below


def test_persistent_grid_is_what_the_gpu_holds_two_thirds_of_it_under_overlap(lib):
    assert grids(lib, BIG)[:2] == [4 * 256, 4 * 256]                                   # resident 6, overlap 4: 6 * 2 / 3 = 4 per CU
    assert grids(lib, BIG, overlap=1)[:2] == [6 * 256, 6 * 256]
    assert grids(lib, BIG, exact=1)[:2] == [6 * 256, 6 * 256]                          # exact mode runs one batch at a time whatever overlap says
    assert grids(lib, BIG, resident_closest=6, resident_any=5)[:2] == [4 * 256, 3 * 256]   # 5 * 2 / 3 = 3
    assert grids(lib, BIG, resident_closest=2, resident_any=3)[:2] == [2 * 256, 2 * 256]   # 2 is not reduced; 3 goes to max(2, 2)
    assert grids(lib, BIG, resident_closest=1, resident_any=0)[:2] == [256, 256]           # at least one per CU
    assert grids(lib, 100)[:2] == [100, 100]                                           # never more workgroups than chunks
    assert grids(lib, BIG, num_cus=304, overlap=1)[:2] == [1824, 1824]


def test_tiny_mode_small_launches_take_one_workgroup_per_cu(lib):
    """Below 4 * num_cus * 2 * (1024 / 64) = 32 768 chunks on 256 CUs."""
    tiny = dict(tiny=1, resident_closest=2, resident_any=2)
    assert grids(lib, 32767, **tiny)[:2] == [256, 256]
    assert grids(lib, 32768, **tiny)[:2] == [512, 512]
    assert grids(lib, 100, **tiny)[:2] == [100, 100]
    assert grids(lib, 32767, **dict(tiny, overlap=1))[:2] == [512, 512]      # only with several batches in flight
    assert grids(lib, 32767, **dict(tiny, exact=1))[:2] == [512, 512]
    assert grids(lib, 32767, **dict(tiny, tiny=0))[:2] == [512, 512]         # only in the tiny-scene mode
    assert grids(lib, 32767, **dict(tiny, resident_any=3))[:2] == [256, 256]  # 3 -> 2 under overlap, then the rule
    assert grids(lib, 32767, **dict(tiny, resident_any=1))[:2] == [256, 256]
    assert grids(lib, 4 * 64 * 2 * 16 - 1, num_cus=64, **tiny)[:2] == [64, 64]      # the threshold scales with the CUs: 8192 on 64
    assert grids(lib, 4 * 64 * 2 * 16, num_cus=64, **tiny)[:2] == [128, 128]


def test_grid_overrides_are_capped_by_the_chunks(lib):
    assert grids(lib, BIG, trace_wgs_per_cu=3)[:2] == [768, 768]
    assert grids(lib, 500, trace_wgs_per_cu=3)[:2] == [500, 500]
    assert grids(lib, BIG, trace_wgs_per_cu=8, overlap=4)[:2] == [2048, 2048]          # as given: no two-thirds share
    assert grids(lib, 1000, trace_wgs_per_cu=2, tiny=1, resident_closest=2, resident_any=2)[:2] == [512, 512]   # ... and no tiny-mode rule
    assert grids(lib, BIG, trace_grid=300)[:2] == [300, 300]
    assert grids(lib, 200, trace_grid=300)[:2] == [200, 200]
    assert grids(lib, BIG, trace_grid=300, trace_wgs_per_cu=3)[:2] == [300, 300]       # the absolute grid wins


def test_shade_wave_grid(lib):
    """One workgroup of four waves per four groups of 8 chunks, at most shade_wgs_per_cu (4) per CU, at least one."""
    assert grids(lib, 1)[2] == 1
    assert grids(lib, 9)[2] == 1            # 2 groups
    assert grids(lib, 33)[2] == 2           # 5 groups
    assert grids(lib, 3200)[2] == 100       # 400 groups, below the cap of 1024
    assert grids(lib, 32736)[2] == 1023     # 4092 groups
    assert grids(lib, 32737)[2] == 1024     # 4093 groups round up to the cap
    assert grids(lib, 32768)[2] == 1024     # 4096 groups: exactly the cap
    assert grids(lib, BIG)[2] == 1024       # capped
    assert grids(lib, BIG, shade_wgs_per_cu=2)[2] == 512
    assert grids(lib, BIG, shade_wgs_per_cu=6, num_cus=64)[2] == 384
    assert grids(lib, BIG, overlap=1, exact=1)[2] == 1024    # (nothing else moves it)


# ---- the bounces

def shade(lib, **kw):
    p = plan(lib, **kw)
    return column(p, "shade", kw.get("bounces", IN_FIELDS["bounces"]))


def test_shade_kernels_of_a_small_frame(lib):
    assert shade(lib) == [FIRST, SORT, SORT, WAVE]                       # rr = 2: k_shade_wave from the bounce after roulette starts
    assert shade(lib, shade_sort=32) == [FIRST, PLAIN_SHADE, PLAIN_SHADE, WAVE]
    assert shade(lib, shade_sort=3, shade_wave=0) == [FIRST, PLAIN_SHADE, PLAIN_SHADE, SORT]
    assert shade(lib, shade_sort=0) == [FIRST, SORT, SORT, WAVE]         # camera rays are never sorted
    assert shade(lib, shade_wave=0) == [FIRST, SORT, SORT, SORT]
    assert shade(lib, shade_wave_from=1) == [FIRST, WAVE, WAVE, WAVE]
    assert shade(lib, shade_wave_from=0) == [FIRST, WAVE, WAVE, WAVE]    # never the first bounce
    assert shade(lib, shade_wave_from=32) == [FIRST, SORT, SORT, SORT]
    assert shade(lib, shade_wave_from=1, shade_wave=0) == [FIRST, SORT, SORT, SORT]
    assert shade(lib, tri_bits=31) == [FIRST, PLAIN_SHADE, PLAIN_SHADE, WAVE]   # no room for a shading class: never sorted
    assert shade(lib, tri_bits=31, shade_sort=1) == [FIRST, PLAIN_SHADE, PLAIN_SHADE, WAVE]
    assert shade(lib, tri_bits=30) == [FIRST, SORT, SORT, WAVE]
    assert shade(lib, min_rr=0) == [FIRST, WAVE, WAVE, WAVE]             # wave_from = 1
    assert shade(lib, min_rr=3) == [FIRST, SORT, SORT, SORT]             # wave_from = 4: beyond the request
    assert shade(lib, bounces=6, min_rr=3) == [FIRST, SORT, SORT, SORT, WAVE, WAVE]
    assert shade(lib, bounces=1) == [FIRST]
    assert shade(lib, bounces=0) == []
    assert shade(lib, bounces=32, min_rr=40) == [FIRST] + [SORT] * 31


def test_automatic_shade_wave_from_takes_the_roulette_bounce_of_large_launches(lib):
    """kWaveRouletteGroupsPerCu (8) groups of 8 chunks per CU: 2048 groups on 256 CUs, counted over a FULL batch of K samples."""
    at = dict(Npad=HEADLINE, spp=8, samples_per_batch=4)            # 4 x 4096 chunks = 2048 groups
    below = dict(Npad=4094 * 256, spp=8, samples_per_batch=4)       # 16 376 chunks = 2047 groups
    assert shade(lib, **at) == [FIRST, SORT, WAVE, WAVE]
    assert shade(lib, **below) == [FIRST, SORT, SORT, WAVE]
    assert shade(lib, Npad=16377 * 256, spp=1) == [FIRST, SORT, WAVE, WAVE]   # 16 377 chunks: a started group counts (2048)
    assert shade(lib, Npad=16376 * 256, spp=1) == [FIRST, SORT, SORT, WAVE]
    assert shade(lib, num_cus=304, **at) == [FIRST, SORT, SORT, WAVE]         # 304 CUs want 2432 groups
    assert shade(lib, num_cus=64, **below) == [FIRST, SORT, WAVE, WAVE]
    assert shade(lib, shade_prefilter=0, **at) == [FIRST, SORT, SORT, WAVE]   # without the prefilter the roulette bounce's chunks are still full
    assert shade(lib, emit_classes=0xFFFF, **at) == [FIRST, SORT, SORT, WAVE]   # every class may emit: the prefilter retires nothing
    assert shade(lib, emit_classes=0x1FFFF, **at) == [FIRST, SORT, SORT, WAVE]  # (the low 16 bits are the classes)
    assert shade(lib, emit_classes=0xFFFE, **at) == [FIRST, SORT, WAVE, WAVE]
    assert shade(lib, emit_classes=0, **at) == [FIRST, SORT, WAVE, WAVE]
    assert shade(lib, min_rr=0, **at) == [FIRST, WAVE, WAVE, WAVE]            # wave_from = 0, and still never the first bounce
    assert shade(lib, shade_wave_from=3, **at) == [FIRST, SORT, SORT, WAVE]   # a given shade_wave_from is taken as it is
    assert shade(lib, shade_wave=0, **at) == [FIRST, SORT, SORT, SORT]
    # the automatic K of the headline frame: 16 x 4096 chunks; and the count follows K down when allocations fail (K = 2: 1024 groups)
    assert shade(lib, Npad=HEADLINE, spp=32) == [FIRST, SORT, WAVE, WAVE]
    p, taken = plan(lib, shrinks=2, Npad=HEADLINE, spp=32)
    assert p.K == 4 and column(p, "shade", 4) == [FIRST, SORT, WAVE, WAVE]
    p, taken = plan(lib, shrinks=3, Npad=HEADLINE, spp=32)
    assert p.K == 2 and column(p, "shade", 4) == [FIRST, SORT, SORT, WAVE]
    p = plan(lib, Npad=HEADLINE, spp=32, clamp=1, available=1)
    assert p.K == 1 and column(p, "shade", 4) == [FIRST, SORT, SORT, WAVE]


def test_tables_that_do_not_fit_lds_select_the_global_memory_variants(lib):
    assert plan(lib).staged == 1
    assert plan(lib, tables_fit_lds=0).staged == 0
    assert plan(lib, stage_lds=0).staged == 0
    assert plan(lib, stage_lds=0, tables_fit_lds=0).staged == 0
    for kw, want in [({}, 1), ({"tables_fit_lds": 0}, 0), ({"stage_lds": 0}, 0)]:     # k_probe follows the same rule
        assert lib.trace_plan_tables_staged(C.byref(make_in(**kw))) == want


def test_what_the_launches_pass_on(lib):
    p = plan(lib)
    assert (p.moments, p.prefilter, p.hit12, p.o12, p.exact) == (0, 1, 1, 1, 0)
    p = plan(lib, moments=1, shade_prefilter=0, hit12=0, o12=0)
    assert (p.moments, p.prefilter, p.hit12, p.o12) == (1, 0, 0, 0)
    assert (plan(lib, hit12=0).hit12, plan(lib, hit12=0).o12, plan(lib, o12=0).hit12, plan(lib, o12=0).o12) == (0, 1, 1, 0)


def test_k_generate_writes_origins_only_where_a_kernel_reads_them(lib):
    assert plan(lib).generate_writes_origins == 0                                          # packet kernel for the camera rays
    assert plan(lib, scene_packet_primary=0).generate_writes_origins == 0                  # k_trace's camera launch
    assert plan(lib, traversal=0).generate_writes_origins == 0                             # (packet kernel still)
    assert plan(lib, scene_packet_primary=0, traversal=0).generate_writes_origins == 1     # k_intersect reads the origin stream
    assert plan(lib, bounces=0).generate_writes_origins == 1                               # nothing traced: as the tap wants them
    assert plan(lib, packet_primary=1, scene_packet_primary=0, traversal=0).generate_writes_origins == 1   # (the RESOLVED packet_primary counts)


# ---- which traversal kernel traces a ray set

def traversal_columns(lib, **kw):
    p = plan(lib, **kw)
    return column(p, "isect", 4), column(p, "occl", 4)


def test_traversal_of_a_batch(lib):
    """The resolved packet_primary for bounce 0 only; packet_shadow for the first N bounces; else k_trace or, with traversal = 0, the plain kernels."""
    assert traversal_columns(lib) == ([PACKET] + [PERSISTENT] * 3, [PERSISTENT] * 4)
    assert traversal_columns(lib, scene_packet_primary=0) == ([PERSISTENT] * 4, [PERSISTENT] * 4)
    assert traversal_columns(lib, scene_packet_primary=0, packet_primary=1) == ([PERSISTENT] * 4, [PERSISTENT] * 4)   # the option itself is not read
    assert traversal_columns(lib, scene_packet_primary=1, packet_primary=0) == ([PACKET] + [PERSISTENT] * 3, [PERSISTENT] * 4)
    assert traversal_columns(lib, traversal=0) == ([PACKET] + [PLAIN] * 3, [PLAIN] * 4)
    assert traversal_columns(lib, traversal=0, scene_packet_primary=0) == ([PLAIN] * 4, [PLAIN] * 4)
    assert traversal_columns(lib, packet_shadow=2) == ([PACKET] + [PERSISTENT] * 3, [PACKET, PACKET, PERSISTENT, PERSISTENT])
    assert traversal_columns(lib, packet_shadow=32, traversal=0, scene_packet_primary=0) == ([PLAIN] * 4, [PACKET] * 4)
    assert traversal_columns(lib, packet_shadow=1, traversal=0) == ([PACKET] + [PLAIN] * 3, [PACKET] + [PLAIN] * 3)
    bt = lambda kind, bounce, **kw: lib.trace_plan_batch_traversal(C.byref(make_in(**kw)), C.c_int64(kind), C.c_int64(bounce))
    assert bt(CAMERA, 0) == PACKET and bt(CLOSEST, 1) == PERSISTENT and bt(ANY_HIT, 0) == PERSISTENT
    assert bt(ANY_HIT, 1, packet_shadow=2) == PACKET and bt(ANY_HIT, 2, packet_shadow=2) == PERSISTENT


def test_traversal_of_a_probe(lib):
    """packet_primary == 1 (the option, not what the upload resolved) and packet_shadow > 0."""
    pt = lambda kind, **kw: lib.trace_plan_probe_traversal(C.byref(make_in(**kw)), C.c_int64(kind))
    assert pt(CLOSEST) == PERSISTENT                                    # automatic packet_primary, resolved to on: still k_trace
    assert pt(CLOSEST, packet_primary=1) == PACKET
    assert pt(CLOSEST, packet_primary=1, scene_packet_primary=0) == PACKET
    assert pt(CLOSEST, packet_primary=0) == PERSISTENT
    assert pt(CLOSEST, traversal=0) == PLAIN
    assert pt(CLOSEST, packet_primary=1, traversal=0) == PACKET
    assert pt(CLOSEST, packet_shadow=3) == PERSISTENT
    assert pt(ANY_HIT) == PERSISTENT
    assert pt(ANY_HIT, packet_shadow=1) == PACKET
    assert pt(ANY_HIT, packet_shadow=1, traversal=0) == PACKET
    assert pt(ANY_HIT, traversal=0) == PLAIN
    assert pt(ANY_HIT, packet_primary=1) == PERSISTENT
    # its persistent grid: the resident capacity (no two-thirds share, no override), capped by the chunks
    pg = lambda any_hit, wgs, **kw: lib.trace_plan_probe_grid(C.byref(make_in(**kw)), C.c_int64(any_hit), C.c_int64(wgs))
    assert pg(0, 4) == 4 and pg(0, 10000) == 1536 and pg(1, 10000, resident_any=5) == 1280 and pg(0, 10000, resident_any=5) == 1536
    assert pg(0, 10000, resident_closest=0) == 256
    assert pg(0, 10000, trace_wgs_per_cu=2, trace_grid=7, overlap=4) == 1536


def test_traversal_of_the_tap(lib):
    """The packet kernel or k_intersect, never k_trace."""
    tt = lambda **kw: lib.trace_plan_tap_traversal(C.byref(make_in(**kw)))
    assert tt() == PACKET
    assert tt(traversal=0) == PACKET
    assert tt(scene_packet_primary=0) == PLAIN
    assert tt(scene_packet_primary=0, traversal=1, packet_primary=1) == PLAIN


def test_traversal_timers(lib):
    timer = lambda how, kind: lib.trace_plan_timer(C.c_int64(how), C.c_int64(kind)).decode()
    assert timer(PACKET, CAMERA) == "intersect_packet"
    assert timer(PERSISTENT, CAMERA) == timer(PERSISTENT, CLOSEST) == timer(PLAIN, CLOSEST) == "intersect"
    assert timer(PACKET, ANY_HIT) == timer(PERSISTENT, ANY_HIT) == timer(PLAIN, ANY_HIT) == "occlusion"
