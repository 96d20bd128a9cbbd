"""The shutter generator's statement (tests/shutter_oracle.py) checked on its own, without a GPU: the ray times
fill [0, 1) evenly, a close state equal to the open one gives the pinhole's (under a lens lens_oracle's) rays bit for bit, a pure
translation keeps every direction and puts every origin on the segment between the two eyes at the ray's own time, and under a lens
every ray passes through the focus point of the camera of its time.  The GPU tests (test_gpu_shutter.py) then hold the kernel to
this statement bit for bit.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_oracle as LO
import shutter_oracle as SO
from conftest import ROOT, bits

F = np.float32
W, H, BY, BH = 24, 10, 3, 6      # rows [3, 9): N = 144, one partly filled chunk
SEEDS = [7, 0x9E3779B9, 0xFFFFFFF0, 123456789]      # (0xFFFFFFF0: gx + seed wraps)
RADIUS, FOCUS = 0.05, 1.9        # as test_lens_cpu.py: 0.05 x the Cornell box's extent; the plane of focus lies inside the box


@pytest.fixture(scope="module")
def cornell():
    from polaris_amd import scenes

    return scenes.SCENES["cornell"](W / H)


@pytest.fixture(scope="module")
def cameras(cornell):
    """The open lens, and the close state of tests/test_gpu_shutter.py (moved and turned) with its lens focused 1.25 x further."""
    lens0 = LO.Lens.from_frustum(cornell.frustum, RADIUS, FOCUS)
    eye1, fr1 = SO.close_camera(cornell)
    lens1 = LO.Lens.from_frustum(fr1, RADIUS, FOCUS * 1.25)
    assert SO.no_negative_zero(cornell.eye, cornell.frustum, eye1, fr1, *lens0.vectors()[1:], *lens1.vectors()[1:])
    return lens0, SO.Close(eye1, fr1, lens1)


# ---- the ray times
@pytest.mark.parametrize("lens", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_ray_times_fill_the_interval_evenly(oracle, seed, lens):
    """4 096 rays of a 64 x 64 block: a bin of an eighth holds 512 on average with sigma = sqrt(4096 / 8 * 7 / 8) = 21.2; the bound
    512 +- 128 is six of them.  (The oracle's PRNG gave 460 ... 551 over these seeds and both draw positions.)"""
    _, _, t = SO.shutter_draws(oracle, 64, 64, seed, lens)
    assert t.dtype == F and t.size == 4096
    assert (t >= 0).all() and (t < 1).all()
    counts = np.histogram(t, bins=8, range=(0.0, 1.0))[0]
    print("seed", hex(seed), "lens", lens, "bins:", counts.tolist())
    assert counts.sum() == 4096 and (np.abs(counts - 512) <= 128).all()


def test_the_time_is_the_draw_after_the_generators_own(oracle):
    """Lens off: the stream's second draw; lens on: its third (the lens point keeps the second, as in k_generate_lens)."""
    s0a, _, ta = SO.shutter_draws(oracle, W, BH, 7, False)
    s0b, s1b, tb = SO.shutter_draws(oracle, W, BH, 7, True)
    l0, l1 = LO.camera_draws(oracle, W, BH, 7)
    assert np.array_equal(bits(s0a), bits(l0)) and np.array_equal(bits(s0b), bits(l0)) and np.array_equal(bits(s1b), bits(l1))
    assert np.array_equal(bits(ta), bits(l1[:, 0])) and not np.array_equal(bits(tb), bits(ta))


# ---- close = open
@pytest.mark.parametrize("seed", SEEDS)
def test_a_close_state_equal_to_the_open_one_gives_the_shutterless_rays(oracle, cornell, cameras, seed):
    lens0, _ = cameras
    same = SO.Close(cornell.eye, cornell.frustum, lens0)
    # lens off: the pinhole's rays, origin = the eye
    rays = SO.shutter_rays(oracle, cornell, same, W, H, BY, BH, seed)
    s0, _ = LO.camera_draws(oracle, W, BH, seed)
    d = LO.pinhole_directions(cornell, W, H, BY, BH, s0)
    assert np.array_equal(bits(rays[:, 4:7]), bits(d))
    assert np.array_equal(bits(rays[:, 0:3]), bits(np.broadcast_to(np.asarray(cornell.eye, F), (W * BH, 3))))
    assert (rays[:, 3] == SO.FLT_MAX).all() and np.array_equal(rays[:, 7], np.arange(W * BH, dtype=F))
    # lens on: lens_oracle's rays
    rays = SO.shutter_rays(oracle, cornell, same, W, H, BY, BH, seed, lens=lens0)
    assert np.array_equal(bits(rays), bits(LO.lens_rays(oracle, cornell, lens0, W, H, BY, BH, seed)))


# ---- a pure translation
@pytest.mark.parametrize("seed", SEEDS)
def test_a_pure_translation_keeps_every_direction_and_moves_the_origin_along_the_segment(oracle, cornell, cameras, seed):
    _, close = cameras
    moved = SO.Close(close.eye1, cornell.frustum)
    rays, det = SO.shutter_rays(oracle, cornell, moved, W, H, BY, BH, seed, details=True)
    s0, _ = LO.camera_draws(oracle, W, BH, seed)
    assert np.array_equal(bits(rays[:, 4:7]), bits(LO.pinhole_directions(cornell, W, H, BY, BH, s0)))
    eye0, eye1, t = np.asarray(cornell.eye, np.float64), moved.eye1.astype(np.float64), det["t"].astype(np.float64)
    exact = eye0[None, :] + (eye1 - eye0)[None, :] * t[:, None]
    # pm_mix rounds the difference, the product and the sum once each: 3 * 2^-24 of the largest magnitude involved bounds it
    scale = max(np.abs(eye0).max(), np.abs(eye1).max(), np.abs(eye1 - eye0).max())
    assert (np.abs(rays[:, 0:3].astype(np.float64) - exact) <= 3 * 2.0 ** -24 * scale).all()
    assert (rays[:, 0:3] != np.asarray(cornell.eye, F)).any()
    assert len(np.unique(bits(rays[:, 0]))) > W * BH // 2      # (every ray its own time)


# ---- under a lens
@pytest.mark.parametrize("seed", SEEDS)
def test_under_a_lens_every_ray_passes_through_the_focus_point_of_its_time(oracle, cornell, cameras, seed):
    """The focus point of the camera at the ray's time is P = eye_t + d ft with the float32 eye_t, d and ft taken exactly; from there
    on the arithmetic is k_generate_lens' with (eye_t, focus_t, axis_t, u_t, v_t) in the lens' place, so the bound is the one
    test_lens_cpu.py derives: 16 * 2^-23 * (max|eye_t| + ft + |u_t| + |v_t|)."""
    lens0, close = cameras
    rays, det = SO.shutter_rays(oracle, cornell, close, W, H, BY, BH, seed, lens=lens0, details=True)
    assert det["on"].all()
    ft = det["ft"].astype(np.float64)
    eye_t = det["eye_t"].astype(np.float64)
    P = eye_t + det["d"].astype(np.float64) * ft[:, None]
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    w = P - o
    miss = np.linalg.norm(w - d * (np.sum(w * d, axis=1) / np.sum(d * d, axis=1))[:, None], axis=1)
    nu, nv = np.linalg.norm(det["u_t"].astype(np.float64), axis=1), np.linalg.norm(det["v_t"].astype(np.float64), axis=1)
    bound = 16 * 2.0 ** -23 * (np.abs(eye_t).max(axis=1) + ft + nu + nv)
    print("largest miss / bound:", float((miss / bound).max()))
    assert (miss <= bound).all()
    assert (np.abs(np.linalg.norm(d, axis=1) - 1) <= 4 * 2.0 ** -24).all()
    # the focus pull: the plane of focus moves from FOCUS to 1.25 FOCUS with the ray's time
    want = FOCUS + (1.25 * FOCUS - FOCUS) * det["t"].astype(np.float64)
    assert (np.abs(det["focus_t"].astype(np.float64) - want) <= 4 * 2.0 ** -24 * 1.25 * FOCUS).all()


# ---- the ABI (beside test_abi.py)
def test_shutter_params_layout_as_the_c_compiler_sees_it(tmp_path):
    from polaris_amd import ctypes_api as T

    fields = ["struct_size", "enabled", "eye1", "frustum1", "focus_distance1", "axis1", "u1", "v1"]
    src = tmp_path / "shutter.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "polaris_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", '
                   "sizeof(PolarisShutterParams), " + ", ".join(f"offsetof(PolarisShutterParams, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "shutter"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [124, 0, 4, 8, 20, 84, 88, 100, 112]
    P = T.ShutterParams
    assert [C.sizeof(P)] + [getattr(P, f).offset for f in fields] == got
    assert P().struct_size == 124 and P().enabled == 0
    p = T.shutter_params((1, 2, 3), np.arange(16), 2.5, (0, 0, 1), (0.1, 0, 0), (0, 0.1, 0))
    assert p.enabled == 1 and list(p.eye1) == [1, 2, 3] and list(p.frustum1) == list(range(16)) and p.focus_distance1 == 2.5 and p.axis1[2] == 1
    assert T.shutter_params().enabled == 0
    assert "polaris_hip_set_shutter" in T.C_ABI_SYMBOLS


def test_set_shutter_refuses_a_null_handle(built):
    from polaris_amd import ctypes_api as T

    lib = T.load_library()
    p = T.shutter_params()
    assert lib.polaris_hip_set_shutter(None, C.byref(p)) == 2       # POLARIS_E_BAD_ARGUMENT
    assert lib.polaris_hip_set_shutter(None, None) == 2


def test_render_cli_refuses_a_shutter_without_camera_frames(built):
    """--shutter is valid only with --frames and without --recolour, within [0, 1]: refused by argparse before the scene is read."""
    import sys

    for flags in (["--shutter", "0.5"], ["--shutter", "0.5", "--frames", "2", "--recolour", "0:1,1,1"], ["--shutter", "1.5", "--frames", "2"],
                  ["--shutter", "-0.1", "--frames", "2"]):
        r = subprocess.run([sys.executable, "-m", "polaris_amd.render", "no_such_scene.obj"] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--shutter" in r.stderr, (flags, r.stderr)
