"""The bloom of the display stage on the CPU (no GPU): polaris_host_bloom -- the restatement the GPU kernels are compared with bit for
bit (tests/test_gpu_bloom.py) -- against an independent numpy statement written from DESIGN.md section 10m (tests/bloom_oracle.py):
bytes, U_1, the full-resolution term and the levels used over odd regions, a sub-block and a hostile plane; the pyramid's conservation
of energy against the same pyramid in float64; the two anchors against polaris_host_display; the parameter checks; and what the bloom
bit changes in the plan of a sync (tests/tools/bloom_plan_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_oracle as BO
from conftest import ROOT
from polaris_amd import ctypes_api as T

F = np.float32
OPERATORS = [T.TONE_REINHARD, T.TONE_REINHARD_WHITE, T.TONE_ACES, T.TONE_HABLE]
# (W, rows, levels asked for, levels used)
REGIONS = [(67, 37, 8, 7), (67, 5, 8, 7), (9, 1, 8, 4), (1, 1, 3, 1), (64, 64, 3, 3)]


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    return host_api


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def hdr_plane(W, H, seed=3):
    """(H, W, 4) float32: a dim log-uniform background with a few pixels and one small lamp far above the threshold."""
    rng = np.random.default_rng(seed)
    p = np.exp(rng.uniform(np.log(1e-3), np.log(0.8), (H, W, 4))).astype(F)
    n = max(1, W * H // 40)
    p[rng.integers(0, H, n), rng.integers(0, W, n), :3] = np.exp(rng.uniform(np.log(1.0), np.log(300.0), (n, 3))).astype(F)
    p[H // 3:H // 3 + 3, W // 2:W // 2 + 4, :3] = F(17.5)
    return p


def hostile_plane(W=23, H=19):
    """Zeros, denormals, negative values, NaN, +-inf and 1e30 among ordinary pixels, some of them side by side."""
    p = hdr_plane(W, H, seed=11)
    odd = np.array([0.0, -0.0, 1e-45, 1e-40, -1e-40, -1.0, -1e30, np.nan, np.inf, -np.inf, 1e30, 3e38, 65536.0, 65537.0], F)
    rng = np.random.default_rng(12)
    p[rng.integers(0, H, 150), rng.integers(0, W, 150), rng.integers(0, 3, 150)] = odd[rng.integers(0, len(odd), 150)]
    p[4:7, 5:9, :3] = F(np.inf)
    p[10, 10:14, :3] = F(np.nan)
    p[12:14, 2:4, :3] = F(1e30)
    p[0, 0, :3] = odd[:3]
    return p


def same(got, want):
    """The restatement's (bytes, U_1, term, L) against the oracle's, bit for bit."""
    assert got[3] == want[3]
    assert got[1].shape == want[1].shape and got[2].shape == want[2].shape
    assert np.array_equal(bits(got[1]), bits(want[1])), "U_1"
    assert np.array_equal(bits(got[2]), bits(want[2])), "term"
    assert np.array_equal(got[0], want[0]), "bytes"


@pytest.mark.parametrize("karis", [0, 1])
@pytest.mark.parametrize("W,rows,levels,used", REGIONS, ids=[f"{w}x{h}" for w, h, _, _ in REGIONS])
def test_restatement_equals_the_numpy_statement(host, W, rows, levels, used, karis):
    p = hdr_plane(W, rows)
    for display in (dict(tone_operator=T.TONE_ACES, srgb=1), dict(tone_operator=T.TONE_HABLE, auto_exposure=1)):
        kw = dict(weight=0.5, exposure=1.25, levels=levels, threshold=1.0, knee=0.5, intensity=0.25, karis=karis, display=display)
        got, want = host.bloom(p, **kw), BO.bloom(p, **kw)
        assert got[3] == used
        same(got, want)
        assert (got[2][..., 3] == 0).all()
        assert display.get("auto_exposure") or got[1][..., :3].max() > 0        # without metering the lamp is above the threshold: something bloomed


def test_levels_used():
    assert [len(BO.level_sizes(w, h, n)) - 1 for w, h, n, _ in REGIONS] == [u for _, _, _, u in REGIONS]
    assert len(BO.level_sizes(1, 1, 8)) - 1 == 1 and len(BO.level_sizes(64, 64, 8)) - 1 == 6


@pytest.mark.parametrize("karis", [0, 1])
def test_rows_outside_the_request_are_never_read(host, karis):
    inner = hdr_plane(67, 25)
    for fill in (np.nan, 1e30):
        p = np.full((37, 67, 4), fill, F)
        p[5:30] = inner
        rgba = np.random.default_rng(5).integers(0, 256, (37, 67, 4)).astype(np.uint8)
        kw = dict(weight=1.0, exposure=1.0, levels=8, karis=karis, display=dict(tone_operator=T.TONE_ACES, auto_exposure=1))
        got = host.bloom(p, block_y=5, block_h=25, rgba=rgba, **kw)
        alone = BO.bloom(inner, **kw)
        assert got[3] == alone[3] == 7
        assert np.array_equal(bits(got[1]), bits(alone[1])) and np.array_equal(bits(got[2]), bits(alone[2]))
        assert np.array_equal(got[0][5:30], alone[0])
        assert np.array_equal(got[0][:5], rgba[:5]) and np.array_equal(got[0][30:], rgba[30:])


@pytest.mark.parametrize("karis", [0, 1])
def test_hostile_plane_stays_finite(host, karis):
    """Every level's D is within [0, 65536]; U_l sums L - l + 1 of them, so U_1 is within [0, 65536 L] and the term within [0, 65536]."""
    p = hostile_plane()
    kw = dict(levels=8, threshold=0.5, knee=0.5, intensity=1.0, karis=karis, display=dict(tone_operator=T.TONE_REINHARD_WHITE))
    got, want = host.bloom(p, **kw), BO.bloom(p, **kw)
    same(got, want)
    L = got[3]
    D, _, _, _ = BO.pyramid(p[..., :3], levels=8, threshold=0.5, knee=0.5, karis=karis)
    for d in D:
        assert np.isfinite(d).all() and d.min() >= 0 and d.max() <= 65536.0
    assert BO.bright(p[..., :3], 1.0, 1.0, 1.0, 0.5, 0.5).max() == F(65536.0 - 0.5)  # the clamp was reached: 65536 less the threshold
    assert np.isfinite(got[1]).all() and got[1].min() >= 0 and got[1].max() <= 65536.0 * L
    assert np.isfinite(got[2]).all() and got[2].min() >= 0 and got[2].max() <= 65536.0


def test_the_pyramid_conserves_energy(host):
    """One pixel (4, 2, 1) at (33, 31) of a black 64 x 64 region, three levels, no threshold: away from the edges the down and up
    filters each conserve the sum, so the term sums to the pixel.  The float32 term's channel sums (added in float64) against the same
    pyramid in float64 numpy: measured relative deviation 4.93e-10 in every channel (the weights are dyadic, so most float32 sums here
    are exact; the float64 pyramid's sums are 4, 2, 1 to 1e-12); the margin is four times that.  (Added in float32 instead, the term's
    sums are 4.0000014, 2.0000007, 1.0000004: that 3.6e-7 is the summation's, not the pyramid's.)"""
    p = np.zeros((64, 64, 4), F)
    p[31, 33, :3] = (4.0, 2.0, 1.0)
    kw = dict(levels=3, threshold=0.0, knee=0.0, karis=0)
    _, _, term, L = host.bloom(p, intensity=1.0, **kw)
    _, _, want, L64 = BO.pyramid(p[..., :3], dtype=np.float64, **kw)
    assert L == L64 == 3
    s32, s64 = term[..., :3].astype(np.float64).sum(axis=(0, 1)), want.sum(axis=(0, 1))
    dev = np.abs(s32 - s64) / s64
    print("bloom conservation: float32 sums", s32, "float64 sums", s64, "relative deviation", dev)
    assert np.allclose(s64, (4.0, 2.0, 1.0), rtol=1e-12, atol=0)
    assert (dev <= 4 * 4.93e-10).all()


@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("op", OPERATORS)
def test_anchors_give_the_display_stage_bytes(host, op, srgb):
    p = hdr_plane(41, 29)                                                       # (displayed values stay below 65536)
    display = dict(tone_operator=op, srgb=srgb, auto_exposure=1)
    plain, _, _ = host.display(p, weight=0.5, exposure=2.0, **display)
    for kw in (dict(intensity=0.0), dict(threshold=65536.0, knee=0.0, intensity=16.0)):
        got = host.bloom(p, weight=0.5, exposure=2.0, display=display, levels=8, **kw)
        assert np.array_equal(got[0], plain), kw
    lit = host.bloom(p, weight=0.5, exposure=2.0, display=display, levels=8)
    assert not np.array_equal(lit[0], plain)                                    # (with the defaults the bytes do change)


# ---- the parameters --------------------------------------------------------------------------------------------------------------
BAD = [dict(enabled=2), dict(karis=2), dict(enabled=0, karis=2), dict(levels=0), dict(levels=9), dict(threshold=-1.0), dict(threshold=65537.0),
       dict(threshold=float("nan")), dict(threshold=float("inf")), dict(knee=-0.1), dict(knee=1.5), dict(knee=float("nan")), dict(intensity=-1.0),
       dict(intensity=16.5), dict(intensity=float("inf")), dict(intensity=float("nan"))]


def test_parameters_are_checked(host):
    lib = host.load()
    assert lib.polaris_host_bloom_check(None) != 0
    assert lib.polaris_host_bloom_check(C.byref(T.bloom_params(1))) == 0
    edge = T.bloom_params(1, levels=8, threshold=65536.0, knee=1.0, intensity=16.0)
    assert lib.polaris_host_bloom_check(C.byref(edge)) == 0
    assert lib.polaris_host_bloom_check(C.byref(T.bloom_params(1, levels=1, threshold=0.0, knee=0.0, intensity=0.0, karis=0))) == 0
    off = T.bloom_params(0, levels=99, threshold=float("nan"), knee=7.0, intensity=-3.0)
    assert lib.polaris_host_bloom_check(C.byref(off)) == 0                      # off: nothing else is looked at
    short = T.bloom_params(1)
    short.struct_size -= 4
    assert lib.polaris_host_bloom_check(C.byref(short)) != 0
    for bad in BAD:
        enabled = bad.get("enabled", 1)
        p = T.bloom_params(enabled, **{k: v for k, v in bad.items() if k != "enabled"})
        assert lib.polaris_host_bloom_check(C.byref(p)) != 0, bad
        if enabled == 1:
            with pytest.raises(ValueError):
                host.bloom(np.ones((2, 2, 4), F), **bad)
    assert T.BLOOM_DEFAULTS == {"levels": 5, "threshold": 1.0, "knee": 0.5, "intensity": 0.25, "karis": 1}
    with pytest.raises(TypeError):
        T.bloom_params(1, radius=3)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "bloom_plan_check.cpp")
LIB = os.path.join(BUILD, "libbloom_plan_check.so")
DISPLAY, AUTO, BLOOM = 32, 64, 128
TONEMAP, METER, EXPOSE, SHOW, GLOW = 4, 5, 6, 7, 8                             # SyncStep, as frame_sync.h numbers them


@pytest.fixture(scope="module")
def plan_lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "frame_sync.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    for fn in (so.bloom_plan_states, so.bloom_plan_max_steps):
        fn.restype = C.c_int64
    so.bloom_plan_bloomed.argtypes, so.bloom_plan_bloomed.restype = [C.c_int64], C.c_int64
    so.bloom_plan_step_timer.argtypes, so.bloom_plan_step_timer.restype = [C.c_int64], C.c_char_p
    for fn in (so.bloom_plan, so.bloom_plan_before):
        fn.argtypes, fn.restype = [C.c_int64, C.c_int64, C.POINTER(C.c_int64)], None
    so.bloom_plan_tail.argtypes, so.bloom_plan_tail.restype = [C.c_int64, C.POINTER(C.c_int64)], None
    return so


def plan_of(fn, state, features):
    out = (C.c_int64 * 32)()
    fn(state, features, out)
    return list(out)[:18]


def test_the_bloom_bit_changes_only_the_tail_of_the_plan(plan_lib):
    assert plan_lib.bloom_plan_step_timer(GLOW) == b"bloom" and plan_lib.bloom_plan_step_timer(SHOW) == b"display"
    assert plan_lib.bloom_plan_max_steps() == 7
    cases = 0
    for state in range(plan_lib.bloom_plan_states()):
        for f in range(128):
            before = plan_of(plan_lib.bloom_plan_before, state, f)
            assert plan_of(plan_lib.bloom_plan, state, f) == before, (state, f)  # the bit off: the plan as it was
            on = plan_of(plan_lib.bloom_plan, state, f | BLOOM)
            n = before[10]
            if not f & DISPLAY:
                assert on == before and not plan_lib.bloom_plan_bloomed(f | BLOOM)  # without the display stage the bit is nothing
            else:
                assert plan_lib.bloom_plan_bloomed(f | BLOOM) and not plan_lib.bloom_plan_bloomed(f)
                assert on[:10] == before[:10] and on[10] == n + 1 <= 7          # planes, clears, PRIOR, the sources: untouched
                assert before[11 + n - 1] == SHOW
                assert on[11:11 + n + 1] == before[11:11 + n - 1] + [GLOW, SHOW]
                assert all(s == -1 for s in on[11 + n + 1:18])
            cases += 1
    assert cases == 6 * 128
    assert max(plan_of(plan_lib.bloom_plan, s, 255)[10] for s in range(6)) == 7


def test_the_plain_sync_runs_the_tail_alone(plan_lib):
    def tail(f):
        out = (C.c_int64 * 8)()
        plan_lib.bloom_plan_tail(f, out)
        return list(out)[:1 + out[0]]

    assert tail(0) == tail(BLOOM) == tail(BLOOM | AUTO) == [1, TONEMAP]
    assert tail(DISPLAY | BLOOM) == [2, GLOW, SHOW] and tail(DISPLAY) == [1, SHOW]
    assert tail(DISPLAY | AUTO | BLOOM) == [4, METER, EXPOSE, GLOW, SHOW] and tail(DISPLAY | AUTO) == [3, METER, EXPOSE, SHOW]
