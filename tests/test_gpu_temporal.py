"""Temporal reuse of the synced frame on the MI355X (include/polaris_hip.h: polaris_hip_set_temporal, POLARIS_AOV_TEMPORAL / _PRIOR,
polaris_hip_reproject_planes).

Bars: k_reproject is bit-equal to the CPU restatement (polaris_host_reproject) on engineered and random planes; on the real path
the PRIOR, TEMPORAL and DENOISED planes are bit-equal to the host chain (reproject, combine, polaris_host_denoise with weight 1)
fed the planes read before and after the move; temporal reuse before any move leaves the frame buffer bytes as they are without
it; it never changes an accumulator or a counter; max_history = 0, resize and upload_scene drop the history."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import gbuffer_oracle as G
import temporal_oracle as TO
import test_temporal_cpu as TC
from conftest import ROOT, bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_denoise import ROOM_MTL, read_png, room_obj, sync, trace, weight_of

pytestmark = pytest.mark.gpu

F = np.float32
TP = T.TEMPORAL_DEFAULTS


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def moved(sc, dx, dy=0.0):
    return dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([dx, dy, 0], F)).astype(F))


def set_cam(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)


# ---- 1. the test entry against the CPU restatement ----------------------------------------------------------------------------
def engineered_cases():
    rng = np.random.default_rng(3)
    W = H = 64
    cases = []
    pe, pf, pg, pa, e, f, g, a = TC.room_pair(W, H)
    cases.append(("disocclusion", TC.history_planes(rng, H, W), pg, pa, pe, pf, g, a, e, f))
    pa2 = pa.copy()
    pa2[..., 3] = G.leaf_word(T.BXDF_ROUGH_CONDUCTOR)
    cases.append(("leaf", TC.history_planes(rng, H, W), pg, pa2, pe, pf, g, a, e, f))
    pg2 = pg.copy()
    pg2[..., :3] *= -1
    cases.append(("normal", TC.history_planes(rng, H, W), pg2, pa, pe, pf, g, a, e, f))
    pg3 = pg.copy()
    pg3[..., 3] *= F(1.25)
    cases.append(("depth", TC.history_planes(rng, H, W), pg3, pa, pe, pf, g, a, e, f))
    hist = TC.history_planes(rng, H, W)
    hist[20:24, 10:14, 1] = np.inf
    hist[40:44, 30:34, 0] = np.nan
    cases.append(("non-finite", hist, g, a, e, f, g, a, e, f))
    be, bf = TO.pinhole((0, 0, -6))
    cases.append(("behind", TC.history_planes(rng, H, W), g, a, be, bf, g, a, e, f))
    f2 = f.copy()
    f2[3, 0] += F(0.01)
    cases.append(("skewed", TC.history_planes(rng, H, W), g, a, e, f2, g, a, e, f))
    for seed in range(4):
        r = np.random.default_rng(50 + seed)
        W2, H2 = (97, 61) if seed % 2 else (64, 64)
        pe, pf = TC.random_move(r)
        e, f = TC.random_move(r)
        pg, pa = TO.trace_planes(pe, pf, W2, H2, TC.ROOM)
        g, a = TO.trace_planes(e, f, W2, H2, TC.ROOM)
        cases.append((f"random{seed}", TC.history_planes(r, H2, W2), pg, pa, pe, pf, g, a, e, f))
    return cases


@pytest.mark.parametrize("params", [TP, dict(max_history=4, normal_threshold=0.5, depth_threshold=0.3),
                                    dict(max_history=4096, normal_threshold=-1.0, depth_threshold=1e6)])
def test_reproject_planes_bit_equal_to_cpu(host, params):
    from polaris_amd.tracer import HipTracer

    tr = HipTracer("planes", 0)
    tr.Init()
    try:
        for name, hist, pg, pa, pe, pf, g, a, e, f in engineered_cases():
            got = tr.reproject_planes(hist, pg, pa, pe, pf, g, a, e, f, **params)
            want = host.reproject(hist, pg, pa, pe, pf, g, a, e, f, **params)
            assert np.array_equal(bits(got), bits(want)), name
    finally:
        tr.Close()


# ---- 2. the real path ---------------------------------------------------------------------------------------------------------
def host_chain(host, hist, g0, a0, sc0, g1, a1, sc1, acc, accumulated, spp, block_y=0, block_h=None, denoise=True):
    prior = host.reproject(hist, g0, a0, sc0.eye, sc0.frustum, g1, a1, sc1.eye, sc1.frustum, **TP)
    tmp = host.temporal_combine(acc, prior, accumulated, spp, block_y=block_y, block_h=block_h)
    den = host.denoise(tmp, F(1), g1, a1, block_y=block_y, block_h=block_h, **T.DENOISE_DEFAULTS) if denoise else None
    return prior, tmp, den


@pytest.mark.parametrize("block", [(0, None), (13, 21)])
def test_real_path_matches_host_chain(host, oracle, block):
    from polaris_amd import scenes

    W, H, spp = 96, 72, 4
    by, bh = block
    rows = slice(by, H if bh is None else by + bh)
    sc0 = scenes.SCENES["cornell"](W / H)
    sc1 = moved(sc0, 0.02, 0.01)
    tr = make_hip_tracer(sc0, W, H)
    try:
        tr.set_denoise()
        tr.set_temporal()
        trace(tr, W, H, spp, base=3)
        sync(tr, W, H, spp)
        hist, g0, a0 = tr.read_aov(T.AOV_TEMPORAL), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        set_cam(tr, sc1)
        fb_before = tr.read_framebuffer()
        trace(tr, W, H, spp, base=5)
        sync(tr, W, H, spp, block_y=by, block_h=bh)
        got = {k: tr.read_aov(k) for k in (T.AOV_PRIOR, T.AOV_TEMPORAL, T.AOV_DENOISED, T.AOV_GUIDE, T.AOV_ALBEDO)}
        acc, fb = tr.read_accumulator(1), tr.read_framebuffer()
    finally:
        tr.Close()
    assert np.array_equal(bits(hist[..., 3]), bits(np.full((H, W), spp, F)))   # (no history at the first view: m = 0, n = spp)
    prior, tmp, den = host_chain(host, hist, g0, a0, sc0, got[T.AOV_GUIDE], got[T.AOV_ALBEDO], sc1, acc, 0, spp, by, bh)
    assert (prior[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(got[T.AOV_PRIOR]), bits(prior))
    assert np.array_equal(bits(got[T.AOV_TEMPORAL][rows]), bits(tmp[rows]))
    assert np.all(got[T.AOV_TEMPORAL][:by, :, 3] == 0)                            # (cleared at the first sync under the camera)
    assert np.array_equal(bits(got[T.AOV_DENOISED][rows, :, :3]), bits(den[rows, :, :3]))
    want_fb = oracle.tonemap(den, 1.0, 1.2).reshape(H, W, 4)
    assert np.array_equal(fb[rows], want_fb[rows])
    outside = np.ones(H, bool)
    outside[rows] = False
    assert np.array_equal(fb[outside], fb_before[outside])                         # rows outside the request keep their bytes


@pytest.mark.parametrize("denoise", [False, True])
def test_before_any_move_bytes_equal_temporal_off(built, denoise):
    from polaris_amd import scenes

    W, H = 80, 64
    sc = scenes.SCENES["cornell"](W / H)
    out = {}
    for on in (False, True):
        tr = make_hip_tracer(sc, W, H)
        try:
            if denoise:
                tr.set_denoise()
            if on:
                tr.set_temporal()
            trace(tr, W, H, 4, base=3)
            sync(tr, W, H, 4)
            trace(tr, W, H, 4, base=4, accumulated=4)
            sync(tr, W, H, 4, accumulated=4, block_y=10, block_h=30)
            out[on] = (tr.read_framebuffer(), tr.read_aov(T.AOV_DENOISED) if denoise else None)
        finally:
            tr.Close()
    assert np.array_equal(out[False][0], out[True][0])
    if denoise:
        assert np.array_equal(bits(out[False][1][10:40]), bits(out[True][1][10:40]))


def test_accumulators_and_counters_do_not_see_temporal_reuse(built):
    from polaris_amd import scenes

    W, H = 80, 64
    sc0 = scenes.SCENES["cornell"](W / H)
    sc1 = moved(sc0, 0.03)
    out = {}
    for on in (False, True):
        tr = make_hip_tracer(sc0, W, H, samples_per_batch=4)
        try:
            if on:
                tr.set_temporal()
            trace(tr, W, H, 16, base=3)
            sync(tr, W, H, 16)
            set_cam(tr, sc1)
            st = trace(tr, W, H, 16, base=5)
            sync(tr, W, H, 16)
            out[on] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st), tr.read_framebuffer())
        finally:
            tr.Close()
    off, on = out[False], out[True]
    assert np.array_equal(bits(off[0]), bits(on[0])) and np.array_equal(bits(off[1]), bits(on[1]))
    assert off[2][:-8] == on[2][:-8]                                       # every counter (device_ms, the last field, is a time)
    assert not np.array_equal(off[3], on[3])


@pytest.mark.parametrize("drop", ["max_history", "resize", "upload"])
def test_history_is_dropped(built, drop):
    from polaris_amd import scenes
    from polaris_amd.tracer import ChangeType, UpdateMode

    W, H = 64, 48
    sc0 = scenes.SCENES["cornell"](W / H)
    sc1 = moved(sc0, 0.02)
    tr = make_hip_tracer(sc0, W, H)
    try:
        tr.set_temporal()
        with pytest.raises(RuntimeError):
            tr.read_aov(T.AOV_PRIOR)                      # before any temporal sync
        trace(tr, W, H, 4)
        sync(tr, W, H, 4)
        set_cam(tr, sc1)
        trace(tr, W, H, 4, base=8)
        sync(tr, W, H, 4)
        assert (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
        if drop == "max_history":
            tr.set_temporal(max_history=0)
            tr.set_temporal()
        elif drop == "resize":
            W, H = 48, 40
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (W, H))
        else:
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc0)
        set_cam(tr, sc0)
        trace(tr, W, H, 4, base=9)
        sync(tr, W, H, 4)
        assert np.all(tr.read_aov(T.AOV_PRIOR) == 0)
    finally:
        tr.Close()


# ---- 3. frame loop and CLI ----------------------------------------------------------------------------------------------------
def test_renderer_frame_loop_reprojects_on_the_primary(host):
    from polaris_amd import scenes

    W, H, spp = 72, 60, 4
    sc0 = scenes.SCENES["cornell"](W / H)
    sc1 = moved(sc0, 0.02)
    r = host.Renderer(sc0, [0, 0], width=W, height=H, spp=spp, seed=5)
    try:
        r.set_temporal()
        r.render()
        hist, g0, a0 = r.read_aov(T.AOV_TEMPORAL), r.read_aov(T.AOV_GUIDE), r.read_aov(T.AOV_ALBEDO)
        r.set_camera(sc1.eye, sc1.frustum)
        rows, _ = r.render()
        fb, acc = r.read()
        prior, tmp = r.read_aov(T.AOV_PRIOR), r.read_aov(T.AOV_TEMPORAL)
        g1, a1 = r.read_aov(T.AOV_GUIDE), r.read_aov(T.AOV_ALBEDO)
    finally:
        r.close()
    assert sum(rows) == H and len(rows) == 2 and min(rows) > 0
    want_prior, want_tmp, _ = host_chain(host, hist, g0, a0, sc0, g1, a1, sc1, acc, 0, spp, denoise=False)
    assert (want_prior[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(prior), bits(want_prior)) and np.array_equal(bits(tmp), bits(want_tmp))


def test_render_cli_frames_match_the_renderer(host, tmp_path):
    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    W, H = 64, 48
    cmd = [sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--width", str(W), "--height", str(H), "--spp", "4",
           "--frames", "3", "--move", "right:0.05", "--temporal", "16", "--denoise", "4", "--out", str(tmp_path / "f.png")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in range(3):
        assert os.path.getsize(tmp_path / f"f_{k:03d}.png") > 0
    sc = host.read_scene(str(tmp_path / "room.obj"), aspect=W / H)
    rd = host.Renderer(sc, [0], width=W, height=H, spp=4, bounces=5, min_rr=3, exposure=1.2, seed=1)
    try:
        rd.set_denoise(iterations=4)
        rd.set_temporal(max_history=16)
        for k in range(3):
            eye, fr = host.camera_move(sc.camera, [("right", 0.05)] * (k + 1), aspect=W / H)
            rd.set_camera(eye, fr)
            rd.render(0)
        fb, _ = rd.read()
        prior = rd.read_aov(T.AOV_PRIOR)
    finally:
        rd.close()
    assert (prior[..., 3] > 0).mean() > 0.5
    assert np.array_equal(read_png(tmp_path / "f_002.png"), fb)


# ---- 4. quality on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell-diffuse", "cornell"])
def test_quality_on_the_device(host, name):
    """The three bars of tests/test_temporal_cpu.py at 512^2 on the device (reference: 256 spp), printed."""
    from polaris_amd import scenes

    N = 512
    sc0 = scenes.SCENES[name]()
    dx = 0.03 / 4                                   # (the same parallax in pixels as 0.03 at 128^2)
    tr = make_hip_tracer(sc0, N, N)
    res = {}
    try:
        for label, step, spp, steps in (("one move, 1 spp", dx, 1, 1), ("8 moves, 1 spp", dx / 3, 1, 8), ("one move, 64 spp", dx, 64, 1)):
            last = moved(sc0, step * steps)
            tr.set_temporal(max_history=0)
            set_cam(tr, last)
            trace(tr, N, N, 256, base=99)
            ref = tr.read_accumulator(1)[..., :3] / 256
            tr.set_denoise()
            tr.set_temporal()
            set_cam(tr, sc0)
            trace(tr, N, N, 64, base=7)
            sync(tr, N, N, 64)
            for k in range(1, steps + 1):
                set_cam(tr, moved(sc0, step * k))
                trace(tr, N, N, spp, base=100 + k)
                sync(tr, N, N, spp)
            tmp_den = tr.read_aov(T.AOV_DENOISED)[..., :3]
            tmp_raw = tr.read_aov(T.AOV_TEMPORAL)[..., :3]
            albedo = tr.read_aov(T.AOV_ALBEDO)
            tr.set_temporal(max_history=0)
            sync(tr, N, N, spp)
            spatial = tr.read_aov(T.AOV_DENOISED)[..., :3]
            raw = tr.read_accumulator(1)[..., :3] / spp
            tr.set_denoise(iterations=0)
            filt = G.filtered_mask(albedo)
            rmse = lambda x: float(np.sqrt(np.mean((x[filt] - ref[filt]) ** 2)))  # noqa: E731
            res[label] = (rmse(tmp_den) / rmse(spatial), rmse(tmp_raw) / rmse(raw))
            print(f"{name} {N}^2 {label}: temporal+atrous / atrous {res[label][0]:.3f}, unfiltered {res[label][1]:.3f}")
    finally:
        tr.Close()
    # (at 512^2 neither scene's a-trous-alone frame carries the 128^2 cornell firefly: bar 1 is the 1.0 of cornell-diffuse)
    assert res["one move, 1 spp"][0] <= 1.0 and res["one move, 1 spp"][1] <= 0.25
    assert res["8 moves, 1 spp"][0] <= 1.0 and res["8 moves, 1 spp"][1] <= 0.3
    assert res["one move, 64 spp"][0] <= 1.05 and res["one move, 64 spp"][1] <= 1.0
