"""The bloom of the display stage on the MI355X (include/polaris_hip.h: polaris_hip_set_bloom, polaris_hip_bloom_planes; DESIGN.md
section 10m).

Bars: k_bloom_down, k_bloom_up, k_bloom_tail and k_display_bloom are bit-equal to the CPU restatement (polaris_host_bloom) on caller
planes -- bytes, U_1 and the levels used -- at the shapes where they can go wrong, with "bloom_fused" 0 and 1 (which are equal to each
other); a bloomed displayed sync of a traced frame is the restatement of its source plane with denoising and temporal reuse on and off;
the accumulators and every counter do not notice it; off, or with the display off, nothing of it runs and the display step is
k_display; set_bloom leaves the exposure state and the temporal history alone; refusals change nothing; and on the Cornell box the
lamp's surroundings gain byte value."""
import dataclasses
import itertools

import numpy as np
import pytest

from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from polaris_amd.tracer import ChangeType, TracerError, UpdateMode
from test_bloom_cpu import hdr_plane, hostile_plane
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

F = np.float32
ACES_AUTO = dict(tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1)


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


@pytest.fixture(scope="module")
def tr(built):
    from polaris_amd import scenes

    t = make_hip_tracer(scenes.SCENES["cornell"](1.0), 16, 16)
    yield t
    t.Close()


def same_as_host(tr, host, plane, **kw):
    """bloom_planes with "bloom_fused" 1 and 0 against the restatement and against each other; returns the restatement's result."""
    want_fb, want_u1, _, want_L = host.bloom(plane, **kw)
    got = {}
    for fused in (1, 0):
        tr.set_option("bloom_fused", fused)
        fb, u1, L = got[fused] = tr.bloom_planes(plane, **kw)
        assert L == want_L and u1.shape == want_u1.shape, (fused, L, want_L)
        assert np.array_equal(bits(u1), bits(want_u1)), (fused, np.argwhere(bits(u1) != bits(want_u1))[:8])
        assert np.array_equal(fb, want_fb), (fused, np.argwhere(fb != want_fb)[:8])
    tr.set_option("bloom_fused", 0)                                              # (the default)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(bits(got[0][1]), bits(got[1][1]))
    return want_fb, want_u1, want_L


# ---- 1. caller planes against the CPU restatement, bit for bit -------------------------------------------------------------------
# (W, rows, levels, levels used): the odd regions; 40 x 40 with 5 levels: level 1 is 20 x 20, so k_bloom_tail starts at level 1 itself;
# 70 x 66: level 1 is 35 x 33 = 1155 pixels, three tiles a side, and the tail starts at level 2
SHAPES = [(67, 37, 8, 7), (67, 5, 8, 7), (9, 1, 8, 4), (1, 1, 3, 1), (64, 64, 3, 3), (40, 40, 5, 5), (70, 66, 8, 7)]


@pytest.mark.parametrize("karis", [0, 1])
@pytest.mark.parametrize("W,rows,levels,used", SHAPES, ids=[f"{w}x{h}" for w, h, _, _ in SHAPES])
def test_planes_equal_the_restatement(tr, host, W, rows, levels, used, karis):
    plane = hdr_plane(W, rows)
    for display, prev in ((dict(tone_operator=T.TONE_HABLE, srgb=0, white=6.0), None), (ACES_AUTO, None), (dict(ACES_AUTO, adapt=0.5), 1.75)):
        _, u1, L = same_as_host(tr, host, plane, weight=0.5, exposure=1.25, levels=levels, karis=karis, display=display, prev_log2E=prev)
        assert L == used and np.isfinite(u1).all()


@pytest.mark.parametrize("karis", [0, 1])
def test_planes_hostile_plane(tr, host, karis):
    _, u1, L = same_as_host(tr, host, hostile_plane(), levels=8, threshold=0.5, knee=0.5, intensity=1.0, karis=karis,
                            display=dict(tone_operator=T.TONE_REINHARD_WHITE))
    assert np.isfinite(u1).all() and u1.min() >= 0 and u1.max() <= 65536.0 * L


def test_planes_sub_block_keeps_the_other_rows_and_never_reads_them(tr, host):
    p = np.full((37, 67, 4), np.nan, F)
    p[30:] = 1e30
    p[5:30] = hdr_plane(67, 25)
    rgba = np.random.default_rng(5).integers(0, 256, (37, 67, 4)).astype(np.uint8)
    fb, u1, L = same_as_host(tr, host, p, block_y=5, block_h=25, rgba=rgba, levels=8, display=ACES_AUTO)
    assert np.array_equal(fb[:5], rgba[:5]) and np.array_equal(fb[30:], rgba[30:]) and np.isfinite(u1).all() and L == 7


def test_planes_refusals(tr):
    p = np.ones((4, 6, 4), F)
    for bad in (dict(levels=0), dict(levels=9), dict(karis=2), dict(threshold=-1.0), dict(threshold=float("nan")), dict(knee=2.0), dict(intensity=17.0),
                dict(display=dict(tone_operator=4)), dict(block_y=4), dict(block_y=1, block_h=4), dict(block_h=0)):
        with pytest.raises(TracerError):
            tr.bloom_planes(p, **bad)
    with pytest.raises(TracerError):
        tr.set_option("bloom_fused", 2)


# ---- 2. the real sync -----------------------------------------------------------------------------------------------------------------
TIMERS = ("bloom", "display", "tonemap")


def cornell(W, H, **options):
    from polaris_amd import scenes

    return make_hip_tracer(scenes.SCENES["cornell"](W / H), W, H, **options)


def source_of(t, denoise, temporal, spp):
    """What the sync's last steps read: DENOISED or TEMPORAL with weight 1, or the frame accumulator with the sync's weight."""
    if denoise:
        return t.read_aov(T.AOV_DENOISED), F(1.0)
    if temporal:
        return t.read_aov(T.AOV_TEMPORAL), F(1.0)
    return t.read_accumulator(1), F(1.0 / spp)


@pytest.mark.parametrize("denoise,temporal", list(itertools.product((0, 1), repeat=2)), ids=lambda v: str(v))
def test_a_bloomed_sync_is_the_restatement_of_its_source(built, host, denoise, temporal):
    W = H = 64
    t = cornell(W, H, time_kernels=1)
    try:
        if denoise:
            t.set_denoise(**T.DENOISE_DEFAULTS)
        if temporal:
            t.set_temporal(**T.TEMPORAL_DEFAULTS)
        t.set_display(1, **ACES_AUTO)
        t.set_bloom(1, **T.BLOOM_DEFAULTS)
        trace(t, W, H, 1)
        sync(t, W, H, 1, exposure=1.2)
        fb = t.read_framebuffer()
        assert {k: t.kernel_ms(k)[1] for k in TIMERS} == {"bloom": 1, "display": 1, "tonemap": 0}
        assert t.kernel_symbol("display").startswith("pol::k_display_bloom<") and t.kernel_symbol("bloom").startswith("pol::k_bloom_")
        src, w = source_of(t, denoise, temporal, 1)
        want = host.bloom(src, weight=w, exposure=1.2, display=ACES_AUTO, **T.BLOOM_DEFAULTS)
        assert np.array_equal(fb, want[0]), np.argwhere(fb != want[0])[:8]
        prev = t.read_exposure()["log2E"]
        sync(t, W, H, 1, exposure=1.2, block_y=16, block_h=32)                   # a block blooms by itself, from the state the frame left
        src, w = source_of(t, denoise, temporal, 1)
        want = host.bloom(src, weight=w, exposure=1.2, block_y=16, block_h=32, rgba=fb, display=ACES_AUTO, prev_log2E=prev, **T.BLOOM_DEFAULTS)
        got = t.read_framebuffer()
        assert np.array_equal(got, want[0]), np.argwhere(got != want[0])[:8]
        assert np.array_equal(got[:16], fb[:16]) and np.array_equal(got[48:], fb[48:])
    finally:
        t.Close()


def test_accumulators_counters_and_launches_do_not_notice_bloom(built):
    W = H = 64

    def run(display, bloom):
        t = cornell(W, H, time_kernels=1)
        try:
            if display:
                t.set_display(1, **ACES_AUTO)
            if bloom:
                t.set_bloom(1, **T.BLOOM_DEFAULTS)
            st = trace(t, W, H, 1)
            sync(t, W, H, 1)
            return dict(fb=t.read_framebuffer(), trace_acc=t.read_accumulator(0), frame_acc=t.read_accumulator(1), stats=bytes(st)[:-8],
                        launches={k: t.kernel_ms(k)[1] for k in TIMERS}, symbol=t.kernel_symbol("display"))
        finally:
            t.Close()

    plain, stored = run(0, 0), run(0, 1)                                         # bloom stored with the display off: not in effect
    shown, lit = run(1, 0), run(1, 1)
    for r in (stored, shown, lit):
        assert np.array_equal(bits(r["trace_acc"]), bits(plain["trace_acc"])) and np.array_equal(bits(r["frame_acc"]), bits(plain["frame_acc"]))
        assert r["stats"] == plain["stats"]
    assert plain["launches"] == stored["launches"] == {"bloom": 0, "display": 0, "tonemap": 1} and np.array_equal(stored["fb"], plain["fb"])
    assert shown["launches"] == {"bloom": 0, "display": 1, "tonemap": 0} and shown["symbol"].startswith("pol::k_display<")
    assert lit["launches"] == {"bloom": 1, "display": 1, "tonemap": 0} and lit["symbol"].startswith("pol::k_display_bloom<")
    assert not np.array_equal(lit["fb"], shown["fb"])


def test_set_bloom_keeps_the_exposure_state_and_the_history_and_survives_a_resize(built, host):
    from polaris_amd import scenes

    W = H = 48
    sc = scenes.SCENES["cornell"](1.0)
    kw = dict(ACES_AUTO, adapt=0.5)
    t = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        t.set_temporal(**T.TEMPORAL_DEFAULTS)
        t.set_bloom(1, **T.BLOOM_DEFAULTS)                                        # accepted and stored with the display off
        trace(t, W, H, 1)
        sync(t, W, H, 1, exposure=1.0)
        assert t.kernel_ms("bloom")[1] == 0 and t.kernel_ms("tonemap")[1] == 1   # not in effect
        t.set_display(1, **kw)                                                   # now it is
        moved = dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([0.3, 0.1, 0.0], F)).astype(F))
        t.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, moved)
        trace(t, W, H, 1)
        sync(t, W, H, 1, exposure=1.0)
        assert t.kernel_ms("bloom")[1] == 1 and t.kernel_symbol("display").startswith("pol::k_display_bloom<")
        before, prior = t.read_exposure(), t.read_aov(T.AOV_PRIOR)
        assert prior[..., 3].max() > 0                                           # a history was reprojected
        t.set_bloom(1, **T.BLOOM_DEFAULTS)                                        # identical bytes: nothing
        t.set_bloom(1, **dict(T.BLOOM_DEFAULTS, levels=3, intensity=0.5))         # a changed call: only the pyramid
        after = t.read_exposure()
        assert all(bits(after[k]) == bits(before[k]) for k in ("avg", "log2E", "E")) and np.array_equal(after["histogram"], before["histogram"])
        sync(t, W, H, 1, exposure=1.0)
        assert np.array_equal(bits(t.read_aov(T.AOV_PRIOR)), bits(prior))        # the history and PRIOR are still there
        want = host.bloom(t.read_aov(T.AOV_TEMPORAL), exposure=1.0, display=kw, prev_log2E=before["log2E"], **dict(T.BLOOM_DEFAULTS, levels=3, intensity=0.5))
        assert np.array_equal(t.read_framebuffer(), want[0])                     # the exposure adapted from the state set_bloom left
        t.set_temporal(max_history=0, normal_threshold=0.9, depth_threshold=0.1)
        t.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (40, 34))   # a resize frees the pyramid; the next sync has its own
        t.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)
        trace(t, 40, 34, 1)
        sync(t, 40, 34, 1, exposure=1.0)
        want = host.bloom(t.read_accumulator(1), exposure=1.0, display=kw, **dict(T.BLOOM_DEFAULTS, levels=3, intensity=0.5))
        assert np.array_equal(t.read_framebuffer(), want[0]) and want[3] == 3
        t.set_display(0)                                                         # the display off: bloom is not in effect
        sync(t, 40, 34, 1, exposure=1.0)
        assert t.kernel_ms("bloom")[1] == 2 and t.kernel_ms("tonemap")[1] == 1
    finally:
        t.Close()


def test_set_bloom_refusals_leave_the_params_and_the_state_unchanged(built, host):
    W = H = 32
    mine = dict(levels=4, threshold=0.8, knee=0.25, intensity=0.5, karis=0)
    t = cornell(W, H)
    try:
        t.set_display(1, **ACES_AUTO)
        t.set_bloom(1, **mine)
        trace(t, W, H, 1)
        sync(t, W, H, 1, exposure=1.0)
        before, fb = t.read_exposure(), t.read_framebuffer()
        for bad in (dict(levels=0), dict(levels=9), dict(karis=2), dict(threshold=-0.5), dict(threshold=1e6), dict(threshold=float("inf")),
                    dict(knee=-0.5), dict(knee=float("nan")), dict(intensity=-1.0), dict(intensity=32.0)):
            with pytest.raises(TracerError):
                t.set_bloom(1, **bad)
        for enabled in (2, 7):
            with pytest.raises(TracerError):
                t.set_bloom(enabled)
        with pytest.raises(TracerError):
            t.set_bloom(0, karis=3)
        p = T.bloom_params(1, **mine)
        p.struct_size += 4
        assert t._lib.polaris_hip_set_bloom(t._h, p) == 2 and t._lib.polaris_hip_set_bloom(t._h, None) == 2
        assert t._lib.polaris_hip_set_bloom(None, T.bloom_params(1)) == 2
        after = t.read_exposure()
        assert all(bits(after[k]) == bits(before[k]) for k in ("avg", "log2E", "E"))
        sync(t, W, H, 1, exposure=1.0)
        want = host.bloom(t.read_accumulator(1), exposure=1.0, display=ACES_AUTO, prev_log2E=before["log2E"], **mine)
        assert np.array_equal(t.read_framebuffer(), want[0]) and np.array_equal(fb, want[0])   # (adapt = 1: the same frame again)
    finally:
        t.Close()


# ---- 3. what bloom is for -------------------------------------------------------------------------------------------------------------
def test_the_lamps_surroundings_gain_byte_value(built, host):
    """The Cornell box, 64 x 64, 1 spp, denoised (for the G-buffer's leaf types), ACES with auto-exposure, bloom's defaults: some pixel
    within 4 pixels of an emitter pixel, not on an emitter, gains byte value, and no channel anywhere loses more than 1 -- first on the
    CPU restatement of the sync's source, then on the device's frames."""
    W = H = 64
    t = cornell(W, H)
    try:
        t.set_denoise(**T.DENOISE_DEFAULTS)
        t.set_display(1, **ACES_AUTO)
        trace(t, W, H, 1)
        sync(t, W, H, 1, exposure=1.0)
        off, src = t.read_framebuffer(), t.read_aov(T.AOV_DENOISED)
        emitter = np.ascontiguousarray(t.read_aov(T.AOV_ALBEDO)[..., 3]).view(np.uint32) == T.BXDF_EMISSIVE
        t.set_bloom(1, **T.BLOOM_DEFAULTS)
        sync(t, W, H, 1, exposure=1.0)
        on = t.read_framebuffer()
    finally:
        t.Close()
    assert 4 < emitter.sum() < W * H // 4
    near = np.zeros_like(emitter)
    for y, x in np.argwhere(emitter):
        near[max(0, y - 4):y + 5, max(0, x - 4):x + 5] = True
    near &= ~emitter
    cpu_off = host.display(src, exposure=1.0, **ACES_AUTO)[0]
    cpu_on = host.bloom(src, exposure=1.0, display=ACES_AUTO, **T.BLOOM_DEFAULTS)[0]
    for a, b in ((cpu_off, cpu_on), (off, on)):
        gain = b[..., :3].astype(np.int32) - a[..., :3].astype(np.int32)
        print(f"\nbloom on the Cornell box: {int((gain[near] > 0).any(axis=-1).sum())} of {int(near.sum())} pixels near the lamp gain, most {int(gain.max())}; "
              f"greatest loss {int(-gain.min())}")
        assert (gain[near] > 0).any() and gain.min() >= -1
    assert np.array_equal(off, cpu_off) and np.array_equal(on, cpu_on)


# ---- 4. the layers above --------------------------------------------------------------------------------------------------------------
def test_renderer_blooms_the_frame_of_its_primary(built, host):
    from polaris_amd import scenes

    W, H, spp = 64, 60, 2
    r = host.Renderer(scenes.SCENES["cornell"](W / H), [0, 0, 0], primary=1, width=W, height=H, spp=spp, exposure=1.2, seed=5)
    try:
        r.set_display(1, **ACES_AUTO)
        r.set_bloom(1, **T.BLOOM_DEFAULTS)
        with pytest.raises(RuntimeError):
            r.set_bloom(1, levels=12)
        r.render()
        fb, acc = r.read()
        want = host.bloom(acc, weight=F(1.0 / spp), exposure=1.2, display=ACES_AUTO, **T.BLOOM_DEFAULTS)[0]
        assert np.array_equal(fb, want)
        assert not np.array_equal(fb, host.display(acc, weight=F(1.0 / spp), exposure=1.2, **ACES_AUTO)[0])
        r.set_bloom(0)
        r.render()
        fb, acc = r.read()
        assert np.array_equal(fb, host.display(acc, weight=F(1.0 / spp), exposure=1.2, **ACES_AUTO)[0])
    finally:
        r.close()


def test_render_py_bloom_flags(built, tmp_path):
    import os

    from polaris_amd import render
    from test_gpu_denoise import ROOM_MTL, room_obj

    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    scene = str(tmp_path / "room.obj")
    out, plain = str(tmp_path / "bloom.png"), str(tmp_path / "plain.png")
    size = ["--width", "48", "--height", "40", "--spp", "2"]
    assert render.main([scene] + size + ["--out", out, "--tonemap", "aces", "--bloom"]) == 0
    assert render.main([scene] + size + ["--out", plain, "--tonemap", "aces"]) == 0
    assert os.path.getsize(out) > 0 and os.path.getsize(plain) > 0
    for bad in (["--bloom"], ["--bloom", "0.5"], ["--bloom-threshold", "2.0"], ["--bloom-levels", "3"], ["--tonemap", "aces", "--bloom-levels", "3"]):
        with pytest.raises(SystemExit):                                          # bloom needs a display flag; its fields need --bloom
            render.main([scene, "--out", plain] + bad)
