"""The display stage on the CPU (no GPU): polaris_host_display -- the restatement the GPU kernels are compared with bit for bit
(tests/test_gpu_display.py) -- against an independent numpy statement written from DESIGN.md section 10l (tests/display_oracle.py):
the bytes of every tone operator and transfer function, the histogram, the exposure (nothing metered, both quantile clips in one
bin, adaptation over five syncs), the anchor against the oracle's own tone-map on a golden frame, the parameter checks, and what
the display bits change in the plan of a sync (tests/tools/display_plan_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_oracle as DO
from conftest import ROOT
from polaris_amd import ctypes_api as T

F = np.float32
OPERATORS = [T.TONE_REINHARD, T.TONE_REINHARD_WHITE, T.TONE_ACES, T.TONE_HABLE]


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    return host_api


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def same_info(got, want):
    return (got["valid"], got["n_metered"]) == (want["valid"], want["n_metered"]) and all(bits(got[k]) == bits(want[k]) for k in ("avg", "log2E", "E"))


def step_ulps(x, j):
    """x moved j float32 steps (x > 0)."""
    return (np.asarray(x, F).view(np.uint32).astype(np.int64) + j).astype(np.uint32).view(F)


def pixels_with_luminance(targets):
    """One rgb per target whose luminance (weight 1) is the target exactly: a grey a few float steps from it with the blue channel, which
    weighs 0.0722, moved up to 40 steps more."""
    out = []
    for t in np.asarray(targets, F):
        j, jb = np.meshgrid(np.arange(-6, 7), np.arange(-40, 41), indexing="ij")
        x = step_ulps(t, j)
        rgb = np.stack([x, x, step_ulps(x, jb)], axis=-1)
        hit = np.argwhere(DO.luminance(rgb, 1.0) == t)
        assert len(hit), t
        out.append(rgb[tuple(hit[0])])
    return np.array(out, F)


def engineered_plane():
    """(H, W, 4) float32 with, as grey pixels: zero, denormals, every bin edge 2^e (1 + k / 8) and up to four float steps either side
    of it, 2^16 and above; then coloured, negative, NaN and infinite channels."""
    e, k = np.meshgrid(np.arange(-16, 17), np.arange(8), indexing="ij")
    edges = (np.exp2(e.astype(np.float64)) * (1 + k / 8)).astype(F).ravel()
    grey = [np.zeros(1, F), np.array([1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 2.0 ** -17, 1.5e-5], F)]
    grey += [step_ulps(edges, j) for j in range(-4, 5)]
    grey += [np.array([65536.0, 65537.0, 1e5, 1e10, 3e38], F), np.geomspace(1e-4, 80.0, 301).astype(F)]
    grey = np.concatenate(grey)
    px = np.concatenate([np.repeat(grey[:, None], 3, axis=1), pixels_with_luminance(np.concatenate([step_ulps(edges, j) for j in (-1, 0, 1)]))])
    rng = np.random.default_rng(7)
    colour = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), (1500, 3))).astype(F)
    special = np.array([[-1.0, 0.5, 0.5], [-0.5, -0.5, -0.5], [-2.0, -3.0, 1e4], [np.nan, 1.0, 1.0], [1.0, np.nan, 0.25], [np.nan] * 3,
                        [np.inf, 1.0, 1.0], [1.0, 1.0, np.inf], [-np.inf, 1.0, 2.0], [np.inf, -np.inf, 0.0], [-0.0, 0.0, -0.0], [1e-3, 0.0, 0.0],
                        [0.0, 1e-3, 0.0], [0.0, 0.0, 1e-3], [0.18, 0.18, 0.18], [1.0, 1.0, 1.0], [4.0, 4.0, 4.0], [3.9999, 4.0001, 4.0]], F)
    px = np.concatenate([px, colour, special])
    W = 97
    H = -(-len(px) // W)
    plane = np.zeros((H * W, 4), F)
    plane[:len(px), :3] = px
    plane[:, 3] = rng.uniform(0, 9, H * W).astype(F)                          # (the fourth channel is not looked at)
    return plane.reshape(H, W, 4)


@pytest.fixture(scope="module")
def plane():
    return engineered_plane()


def test_the_engineered_plane_reaches_both_sides_of_every_bin_edge(plane):
    b = DO.bins_of(DO.luminance(plane[..., :3], 1.0)).ravel()
    assert set(range(256)) <= set(b.tolist()) and -1 in b                     # every bin, and pixels that are not metered
    L = DO.luminance(plane[..., :3], 1.0).ravel()
    e, k = np.meshgrid(np.arange(-16, 16), np.arange(8), indexing="ij")
    for edge in (np.exp2(e.astype(np.float64)) * (1 + k / 8)).astype(F).ravel():
        assert np.any(L == edge) and np.any(L == step_ulps(edge, -1)) and np.any(L == step_ulps(edge, 1)), edge
    assert np.any(L == F(65536.0)) and np.any(L == step_ulps(F(65536.0), -1))


# ---- bytes, histogram and exposure against the numpy statement ---------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("op", OPERATORS)
@pytest.mark.parametrize("auto", [0, 1])
def test_bytes_histogram_and_exposure_match_independent_restatement(host, plane, op, srgb, auto):
    for weight, exposure, white in ((1.0, 1.0, 4.0), (0.25, 1.7, 1.5), (3.0, 0.01, 11.2)):
        kw = dict(weight=weight, exposure=exposure, tone_operator=op, srgb=srgb, white=white, auto_exposure=auto, key=0.18, low_permille=500,
                  high_permille=950, compensation_ev=0.5 if weight == 3.0 else 0.0)
        got_fb, got_hist, got_info = host.display(plane, **kw)
        want_fb, want_hist, want_info = DO.display(plane, **kw)
        assert np.array_equal(got_hist, want_hist)
        assert same_info(got_info, want_info), (got_info, want_info)
        diff = np.argwhere(got_fb != want_fb)
        assert len(diff) == 0, (diff[:5], [plane[tuple(d[:2])] for d in diff[:5]])
        if auto:
            assert got_info["valid"] == 1 and got_info["n_metered"] == int(got_hist.sum()) > 3000


def test_rows_outside_the_request_keep_their_bytes_and_are_not_metered(host, plane):
    H = plane.shape[0]
    rgba = np.random.default_rng(3).integers(0, 256, plane.shape, dtype=np.uint8)
    kw = dict(block_y=5, block_h=H - 11, rgba=rgba, tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1)
    got_fb, got_hist, got_info = host.display(plane, **kw)
    want_fb, want_hist, want_info = DO.display(plane, **kw)
    assert np.array_equal(got_fb, want_fb) and np.array_equal(got_hist, want_hist) and same_info(got_info, want_info)
    assert np.array_equal(got_fb[:5], rgba[:5]) and np.array_equal(got_fb[H - 6:], rgba[H - 6:])
    assert np.array_equal(got_hist, DO.histogram(plane[5:H - 6, :, :3], 1.0))


def test_histogram_bins_come_from_the_float_bits(host):
    """One pixel per bin at its lower edge, one just under it: the counts are exact and 2^16 and above land in bin 255."""
    e, k = np.meshgrid(np.arange(-16, 16), np.arange(8), indexing="ij")
    edges = (np.exp2(e.astype(np.float64)) * (1 + k / 8)).astype(F).ravel()
    p = np.zeros((1, 256 + 3, 4), F)
    p[0, :256, 1] = edges / F(0.7152)                                         # green only: L = 0.7152 g
    p[0, 256:, 1] = [1e5, 1e9, 2.0 ** -17]
    L = DO.luminance(p[..., :3], 1.0)
    _, hist, info = host.display(p, auto_exposure=1)
    assert np.array_equal(hist, DO.histogram(p[..., :3], 1.0))
    assert info["n_metered"] == int(np.sum(np.isfinite(L) & (L >= F(2.0 ** -16)))) and hist[255] >= 2


def test_nothing_metered_leaves_the_state_alone(host):
    for p in (np.zeros((4, 9, 4), F), np.full((4, 9, 4), np.nan, F), np.full((3, 5, 4), 1e-6, F), np.full((2, 2, 4), -1.0, F)):
        fb, hist, info = host.display(p, auto_exposure=1)
        assert hist.sum() == 0 and same_info(info, DO.display(p, auto_exposure=1)[2])
        assert (info["valid"], info["n_metered"], float(info["E"])) == (0, 0, 1.0)
        assert np.array_equal(fb, DO.display(p, auto_exposure=1)[0])
        fb, hist, info = host.display(p, auto_exposure=1, prev_log2E=-2.5)
        want = DO.display(p, auto_exposure=1, prev_log2E=-2.5)
        assert same_info(info, want[2]) and np.array_equal(fb, want[0])
        assert info["valid"] == 1 and bits(info["log2E"]) == bits(F(-2.5)) and abs(float(info["E"]) - 2 ** -2.5) < 1e-6


def test_both_quantile_clips_inside_one_bin(host):
    """Every pixel in one bin: the window [0.3 N, 0.7 N) is cut out of that bin at both ends and avg is the bin's value."""
    p = np.full((30, 30, 4), 0.75, F)
    for low, high in ((300, 700), (0, 1), (999, 1000), (0, 1000)):
        kw = dict(auto_exposure=1, low_permille=low, high_permille=high, key=0.18)
        _, hist, info = host.display(p, **kw)
        want = DO.display(p, **kw)[2]
        assert same_info(info, want), (low, high, info, want)
        b = int(np.argmax(hist))
        assert hist[b] == 900 and abs(float(info["avg"]) - float(DO.bin_values()[b])) < 1e-6
    two = p.copy()
    two[:10] = 0.01                                                            # 300 dark pixels, 600 bright: the window takes from both bins
    kw = dict(auto_exposure=1, low_permille=200, high_permille=900)
    assert same_info(host.display(two, **kw)[2], DO.display(two, **kw)[2])
    one = np.full((1, 1, 4), 2.0, F)                                           # one pixel: N high / 1000 = 0, the window is that pixel
    assert same_info(host.display(one, auto_exposure=1)[2], DO.display(one, auto_exposure=1)[2])
    assert host.display(one, auto_exposure=1)[2]["n_metered"] == 1


def test_adaptation_over_five_syncs(host):
    """A light switched on: the state moves `adapt` of the way to the target at every sync, the first sync snaps."""
    rng = np.random.default_rng(11)
    base = np.exp(rng.normal(-1.0, 1.2, (24, 31, 4))).astype(F)
    scales = [1.0, 64.0, 64.0, 64.0, 0.5]
    for adapt in (0.25, 1.0):
        prev_got = prev_want = None
        targets = []
        for s in scales:
            kw = dict(auto_exposure=1, adapt=adapt, tone_operator=T.TONE_HABLE, srgb=1, compensation_ev=-0.5)
            fb, _, got = host.display(base * F(s), prev_log2E=prev_got, **kw)
            want_fb, _, want = DO.display(base * F(s), prev_log2E=prev_want, **kw)
            assert same_info(got, want) and np.array_equal(fb, want_fb), (adapt, s)
            targets.append(float(host.display(base * F(s), **kw)[2]["log2E"]))   # (without a state: the target itself)
            prev_got, prev_want = got["log2E"], want["log2E"]
        if adapt == 1.0:
            assert abs(float(prev_got) - targets[-1]) < 1e-6
        assert abs((targets[1] - targets[0]) + 6.0) < 0.2                       # 64 times the light: about six stops down


def test_clamps_and_compensation(host):
    p = np.full((8, 8, 4), 0.18, F)
    assert abs(float(host.display(p, auto_exposure=1)[2]["log2E"])) < 0.1      # middle grey metered at key 0.18: about E = 1
    assert float(host.display(p, auto_exposure=1, compensation_ev=2.0)[2]["log2E"]) == pytest.approx(2.0, abs=0.1)
    assert float(host.display(p * F(1e-4), auto_exposure=1, max_ev=3.0)[2]["log2E"]) == 3.0
    assert float(host.display(p * F(1e4), auto_exposure=1, min_ev=-1.5)[2]["log2E"]) == -1.5


def test_curves_have_their_shape(host):
    """White maps to 255 with REINHARD_WHITE and HABLE at white; every curve is monotone over [0, white]."""
    x = np.linspace(0, 4, 400, dtype=F)
    p = np.zeros((1, 400, 4), F)
    p[0, :, :3] = x[:, None]
    for op in OPERATORS:
        for srgb in (0, 1):
            fb = host.display(p, tone_operator=op, srgb=srgb, white=4.0)[0][0, :, 0].astype(int)
            assert np.all(np.diff(fb) >= 0) and fb[0] == 0
            if op in (T.TONE_REINHARD_WHITE, T.TONE_HABLE):
                assert fb[-1] >= 254


# ---- the anchor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_diffuse_32", "cornell_layered_32", "materials_32"])
def test_reinhard_gamma_without_auto_exposure_is_the_oracles_tonemap(host, oracle, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    acc = np.zeros(z["accum"].shape[:2] + (4,), F)
    acc[..., :3] = z["accum"]
    H, W = acc.shape[:2]
    for weight, exposure in ((1.0, 1.0), (1.0 / 6.0, 1.0), (0.125, 2.5), (7.0, 0.3)):
        want = oracle.tonemap(acc, weight, exposure).reshape(H, W, 4)
        got = host.display(acc, weight=weight, exposure=exposure, tone_operator=T.TONE_REINHARD, srgb=0, auto_exposure=0)[0]
        assert np.array_equal(got, want)
        assert np.array_equal(got, DO.display(acc, weight=weight, exposure=exposure)[0])
    assert len(np.unique(want)) > 20                                            # (a frame with content)


# ---- the parameter checks ---------------------------------------------------------------------------------------------------------
BAD = [dict(tone_operator=4), dict(srgb=2), dict(auto_exposure=2), dict(white=0.0), dict(white=float("nan")), dict(white=1e7), dict(white=-1.0),
       dict(auto_exposure=1, key=0.0), dict(auto_exposure=1, key=float("inf")), dict(auto_exposure=1, compensation_ev=25.0),
       dict(auto_exposure=1, compensation_ev=float("nan")), dict(auto_exposure=1, low_permille=950, high_permille=950),
       dict(auto_exposure=1, low_permille=960, high_permille=950), dict(auto_exposure=1, high_permille=1001), dict(auto_exposure=1, min_ev=-25.0),
       dict(auto_exposure=1, max_ev=25.0), dict(auto_exposure=1, min_ev=2.0, max_ev=1.0), dict(auto_exposure=1, adapt=0.0),
       dict(auto_exposure=1, adapt=1.5), dict(auto_exposure=1, adapt=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_parameters_out_of_range_are_refused(host, bad):
    with pytest.raises(ValueError):
        host.display(np.ones((2, 2, 4), F), **bad)


def test_rows_and_struct_size_are_checked(host):
    p = np.ones((4, 3, 4), F)
    for kw in (dict(block_y=4), dict(block_y=2, block_h=3), dict(block_h=0)):
        with pytest.raises(ValueError):
            host.display(p, **kw)
    lib, fb = host.load(), np.zeros((4, 3, 4), np.uint8)
    prm = T.display_params(1)
    assert lib.polaris_host_display(p.ctypes.data, 3, 4, 0, 4, 1.0, 1.0, C.byref(prm), None, fb.ctypes.data, None, None) == 0
    prm.struct_size -= 4
    assert lib.polaris_host_display(p.ctypes.data, 3, 4, 0, 4, 1.0, 1.0, C.byref(prm), None, fb.ctypes.data, None, None) == 2
    off = T.display_params(0)
    assert lib.polaris_host_display(p.ctypes.data, 3, 4, 0, 4, 1.0, 1.0, C.byref(off), None, fb.ctypes.data, None, None) == 2
    assert T.DISPLAY_DEFAULTS["key"] == 0.18 and (T.DISPLAY_DEFAULTS["low_permille"], T.DISPLAY_DEFAULTS["high_permille"]) == (500, 950)
    assert T.DISPLAY_DEFAULTS["adapt"] == 1.0


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "display_plan_check.cpp")
LIB = os.path.join(BUILD, "libdisplay_plan_check.so")
DISPLAY, AUTO = 32, 64
TONEMAP, METER, EXPOSE, SHOW = 4, 5, 6, 7                                      # SyncStep, as frame_sync.h numbers them


@pytest.fixture(scope="module")
def plan_lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "frame_sync.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    so.display_plan_states.restype = C.c_int64
    so.display_plan_step_timer.restype = C.c_char_p
    for fn in (so.display_plan, so.display_plan_before):
        fn.argtypes, fn.restype = [C.c_int64, C.c_int64, C.POINTER(C.c_int64)], None
    so.display_plan_tail.argtypes, so.display_plan_tail.restype = [C.c_int64, C.POINTER(C.c_int64)], None
    so.display_plan_step_timer.argtypes = [C.c_int64]
    return so


def plan_of(fn, state, features):
    out = (C.c_int64 * 18)()
    fn(state, features, out)
    return list(out)


def test_the_display_bits_change_only_the_tail_of_the_plan(plan_lib):
    assert [plan_lib.display_plan_step_timer(s) for s in (TONEMAP, METER, EXPOSE, SHOW)] == [b"tonemap", b"meter", b"expose", b"display"]
    cases = 0
    for state in range(plan_lib.display_plan_states()):
        for f in range(32):
            before = plan_of(plan_lib.display_plan_before, state, f)
            off = plan_of(plan_lib.display_plan, state, f)
            assert off == before, (state, f)                                    # the bits off: the plan as it was
            assert plan_of(plan_lib.display_plan, state, f | AUTO) == before    # auto-exposure without the stage is nothing
            n = before[10]
            assert before[11 + n - 1] == TONEMAP and n <= 4
            for extra, tail in ((DISPLAY, [SHOW]), (DISPLAY | AUTO, [METER, EXPOSE, SHOW])):
                on = plan_of(plan_lib.display_plan, state, f | extra)
                assert on[:10] == before[:10], (state, f, extra)                 # planes, clears, PRIOR, the sources: untouched
                steps_before, steps_on = before[11:11 + n], on[11:11 + on[10]]
                assert steps_on == steps_before[:-1] + tail and on[10] <= on[17]
                assert all(s == -1 for s in on[11 + on[10]:17])
            cases += 1
    assert cases == 6 * 32
    states = {tuple(plan_of(plan_lib.display_plan_before, s, 31)) for s in range(6)}
    assert len(states) >= 4                                                     # (the states really differ in the plan they give)


def test_the_plain_sync_runs_the_tail_alone(plan_lib):
    def tail(f):
        out = (C.c_int64 * 4)()
        plan_lib.display_plan_tail(f, out)
        return list(out)

    assert tail(0) == [1, TONEMAP, -1, -1] and tail(AUTO) == [1, TONEMAP, -1, -1]
    assert tail(DISPLAY) == [1, SHOW, -1, -1] and tail(DISPLAY | AUTO) == [3, METER, EXPOSE, SHOW]
