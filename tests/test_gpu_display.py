"""The display stage on the MI355X (include/polaris_hip.h: polaris_hip_set_display, polaris_hip_read_exposure,
polaris_hip_display_planes).

Bars: k_meter, k_expose and k_display are bit-equal to the CPU restatement (polaris_host_display) on caller planes -- bytes, histogram
and exposure -- at the shapes where they can go wrong; REINHARD with pow(1 / 2.2) and auto-exposure off gives the frame-buffer bytes of
the plain sync with every other feature on and off; the accumulators and every counter do not notice the stage; with it off its
kernels never run; auto-exposure holds the displayed frame's mean byte value while every emitter is made 64 times brighter; the
exposure state survives a camera move and a material edit and is reset by a resize and by a changed set_display; refusals change
nothing."""
import dataclasses
import itertools

import numpy as np
import pytest

import display_oracle as DO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from polaris_amd.tracer import ChangeType, TracerError, UpdateMode
from test_display_cpu import engineered_plane, same_info
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

F = np.float32
OPERATORS = [T.TONE_REINHARD, T.TONE_REINHARD_WHITE, T.TONE_ACES, T.TONE_HABLE]
TIMERS = ("meter", "expose", "display", "tonemap")


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


def radiance_plane(rng, H, W):
    """Log-normal radiance over twenty stops with zeros, negative, NaN and infinite channels sprinkled in."""
    p = np.exp(rng.normal(-1.0, 3.0, (H, W, 4))).astype(F)
    flat = p.reshape(-1, 4)
    n = len(flat)
    for k, v in enumerate((0.0, -0.5, np.nan, np.inf, 1e-7, 7e4)):
        flat[rng.integers(0, n, max(1, n // 40)), k % 3] = v
    return p


def same_as_host(tr, host, plane, **kw):
    got_fb, got_hist, got_info = tr.display_planes(plane, **kw)
    want_fb, want_hist, want_info = host.display(plane, **kw)
    assert np.array_equal(got_hist, want_hist), np.argwhere(got_hist != want_hist)[:8]
    assert same_info(got_info, want_info), (got_info, want_info)
    assert np.array_equal(got_fb, want_fb), np.argwhere(got_fb != want_fb)[:8]
    return got_fb, got_hist, got_info


# ---- 1. caller planes against the CPU restatement, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("op", OPERATORS)
def test_planes_67x5_every_operator_and_transfer(tr, host, op, srgb):
    plane = radiance_plane(np.random.default_rng(10 * op + srgb), 5, 67)       # a partial last workgroup; 335 pixels are no wave multiple
    for auto in (0, 1):
        fb, hist, info = same_as_host(tr, host, plane, weight=0.5, exposure=1.3, tone_operator=op, srgb=srgb, white=3.0, auto_exposure=auto,
                                      compensation_ev=0.25)
        assert info["valid"] == auto and int(hist.sum()) == info["n_metered"] and (info["n_metered"] > 250) == bool(auto)
        assert np.all(fb[..., 3] == 255) and len(np.unique(fb[..., :3])) > 100


def test_planes_sub_block_keeps_the_other_rows_and_does_not_meter_them(tr, host):
    rng = np.random.default_rng(2)
    plane = radiance_plane(rng, 5, 67)
    plane[0], plane[4] = 3e4, 2e-5                                              # what the rows outside would do to the histogram
    rgba = rng.integers(0, 256, (5, 67, 4), dtype=np.uint8)
    fb, hist, info = same_as_host(tr, host, plane, block_y=1, block_h=3, rgba=rgba, tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1)
    assert np.array_equal(fb[0], rgba[0]) and np.array_equal(fb[4], rgba[4]) and not np.array_equal(fb[1:4], rgba[1:4])
    assert info["n_metered"] <= 3 * 67 and info["n_metered"] == int(hist.sum())
    whole = tr.display_planes(plane, tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1)[2]
    assert whole["n_metered"] > info["n_metered"]


def test_planes_one_pixel_per_bin(tr, host):
    e, k = np.meshgrid(np.arange(-16, 16), np.arange(8), indexing="ij")
    mid = (np.exp2(e.astype(np.float64)) * (1 + (k + 0.5) / 8)).astype(F).ravel()
    plane = np.zeros((1, 256, 4), F)
    plane[0, :, :3] = mid[:, None]
    _, hist, info = same_as_host(tr, host, plane, auto_exposure=1, low_permille=0, high_permille=1000)
    assert np.all(hist == 1) and info["n_metered"] == 256
    assert abs(float(info["avg"]) - float(DO.bin_values().astype(np.float64).mean())) < 1e-5   # the mean of the 256 bins' values


def test_planes_every_pixel_in_one_bin(tr, host):
    plane = np.full((300, 300, 4), 0.75, F)                                     # 90 000 atomic adds to one word, 88 workgroups
    _, hist, info = same_as_host(tr, host, plane, auto_exposure=1, low_permille=300, high_permille=700, tone_operator=T.TONE_HABLE)
    assert int(hist.max()) == 90000 and int(hist.sum()) == 90000 and info["n_metered"] == 90000


def test_planes_with_no_metered_pixel(tr, host):
    for plane in (np.zeros((5, 67, 4), F), np.full((5, 67, 4), np.nan, F), np.full((3, 9, 4), 1e-6, F)):
        _, hist, info = same_as_host(tr, host, plane, auto_exposure=1)
        assert hist.sum() == 0 and (info["valid"], info["n_metered"], float(info["E"])) == (0, 0, 1.0)
        _, _, info = same_as_host(tr, host, plane, auto_exposure=1, prev_log2E=1.75)
        assert info["valid"] == 1 and bits(info["log2E"]) == bits(F(1.75))


def test_planes_adaptation_and_the_engineered_plane(tr, host):
    plane = engineered_plane()                                                  # (every bin edge and a float step either side of it)
    prev = None
    for scale, adapt in ((1.0, 0.5), (64.0, 0.5), (64.0, 0.25), (0.125, 1.0), (1.0, 0.1)):
        _, _, info = same_as_host(tr, host, plane, weight=scale, auto_exposure=1, adapt=adapt, prev_log2E=prev, tone_operator=T.TONE_REINHARD_WHITE,
                                  white=2.0)
        prev = info["log2E"]
    for op, srgb in itertools.product(OPERATORS, (0, 1)):
        same_as_host(tr, host, plane, tone_operator=op, srgb=srgb, exposure=0.7)


def test_planes_refusals(tr):
    p = np.ones((4, 6, 4), F)
    for bad in (dict(tone_operator=4), dict(srgb=2), dict(white=0.0), dict(auto_exposure=1, adapt=0.0), dict(auto_exposure=1, low_permille=600, high_permille=600),
                dict(auto_exposure=1, key=-1.0), dict(block_y=4), dict(block_y=1, block_h=4), dict(block_h=0)):
        with pytest.raises(TracerError):
            tr.display_planes(p, **bad)
    with pytest.raises(TracerError):
        tr.read_exposure()                                                       # (display_planes touches no tracer state)


# ---- 2. the anchor and the invariants on a traced frame ------------------------------------------------------------------------------
def traced(features, display, W=64, H=64, spp=4):
    """Trace the Cornell box at W x H, sync with the features (denoise, temporal, variance) and the display fields (None: off); what
    the device holds afterwards."""
    from polaris_amd import scenes

    denoise, temporal, variance = features
    t = make_hip_tracer(scenes.SCENES["cornell"](W / H), W, H, time_kernels=1)
    try:
        if variance:
            t.set_variance(**T.VARIANCE_DEFAULTS)
        if denoise:
            t.set_denoise(**T.DENOISE_DEFAULTS)
        if temporal:
            t.set_temporal(**T.TEMPORAL_DEFAULTS)
        if display is not None:
            t.set_display(1, **display)
        st = trace(t, W, H, spp)
        sync(t, W, H, spp)
        return dict(fb=t.read_framebuffer(), trace_acc=t.read_accumulator(0), frame_acc=t.read_accumulator(1), stats=bytes(st)[:-8],
                    launches={k: t.kernel_ms(k)[1] for k in TIMERS})
    finally:
        t.Close()


@pytest.mark.parametrize("features", list(itertools.product((0, 1), repeat=3)), ids=lambda f: "denoise%d-temporal%d-variance%d" % f)
def test_reinhard_gamma_without_auto_exposure_gives_the_plain_syncs_bytes(built, features):
    off = traced(features, None)
    on = traced(features, dict(tone_operator=T.TONE_REINHARD, srgb=0, auto_exposure=0))
    assert np.array_equal(on["fb"], off["fb"]) and len(np.unique(off["fb"])) > 50
    for k in ("trace_acc", "frame_acc"):
        assert np.array_equal(bits(on[k]), bits(off[k]))                        # the accumulators and every counter do not notice the stage
    assert on["stats"] == off["stats"]
    assert off["launches"] == {"meter": 0, "expose": 0, "display": 0, "tonemap": 1}
    assert on["launches"] == {"meter": 0, "expose": 0, "display": 1, "tonemap": 0}
    auto = traced(features, dict(tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1))
    assert auto["launches"] == {"meter": 1, "expose": 1, "display": 1, "tonemap": 0}
    for k in ("trace_acc", "frame_acc"):
        assert np.array_equal(bits(auto[k]), bits(off[k]))
    assert auto["stats"] == off["stats"] and not np.array_equal(auto["fb"], off["fb"])


def test_a_displayed_sync_is_the_restatement_of_its_accumulator(built, host):
    """The real path with nothing else on: the bytes and the exposure of the sync are polaris_host_display's of the frame accumulator."""
    from polaris_amd import scenes

    W, H, spp = 64, 48, 2
    t = make_hip_tracer(scenes.SCENES["cornell"](W / H), W, H)
    try:
        kw = dict(tone_operator=T.TONE_HABLE, srgb=1, white=6.0, auto_exposure=1, compensation_ev=0.5)
        t.set_display(1, **kw)
        trace(t, W, H, spp)
        sync(t, W, H, spp, exposure=1.2)
        want_fb, want_hist, want_info = host.display(t.read_accumulator(1), weight=F(1.0 / spp), exposure=1.2, **kw)
        got = t.read_exposure()
        assert np.array_equal(t.read_framebuffer(), want_fb) and np.array_equal(got["histogram"], want_hist) and same_info(got, want_info)
        fb = t.read_framebuffer()
        sync(t, W, H, spp, exposure=1.2, block_y=10, block_h=7)                  # a block: only its rows are metered and written
        want_fb, want_hist, want_info = host.display(t.read_accumulator(1), weight=F(1.0 / spp), exposure=1.2, block_y=10, block_h=7, rgba=fb, **kw)
        got = t.read_exposure()
        assert np.array_equal(t.read_framebuffer(), want_fb) and np.array_equal(got["histogram"], want_hist) and same_info(got, want_info)
    finally:
        t.Close()


# ---- 3. auto-exposure's reason to exist ----------------------------------------------------------------------------------------------
def brighter(sc, factor):
    n = sc.material_nodes.copy()
    emissive = n["type"] == T.BXDF_EMISSIVE
    assert emissive.any()
    n["k"][emissive, :3] *= F(factor)
    return n


def test_auto_exposure_holds_the_frame_while_the_lights_get_64_times_brighter(built, host):
    """Every emitter times 64 through update_materials.  Displayed with auto-exposure the frame's mean byte value stays within a band of
    the unscaled frame's; the band is what the CPU restatement itself moves by when the unscaled accumulator is multiplied by 64
    exactly (the histogram's granularity), plus 2 byte values for the two frames being different 1 spp traces.  Without the stage the
    frame saturates: a channel at or above middle grey (c >= 0.18, byte 108) is at c >= 11.5, byte 245, or above.
    Measured (profiles/display_quality.txt): displayed means 61.55 and 61.56 (band 2.01), plain means 46.60 and 153.41."""
    from polaris_amd import scenes

    W = H = 64
    sc = scenes.cornell_box("layered")
    kw = dict(tone_operator=T.TONE_REINHARD, srgb=0, auto_exposure=1)
    out = {}
    t = make_hip_tracer(sc, W, H)
    try:
        for name, factor in (("base", 1.0), ("x64", 64.0)):
            if factor != 1.0:
                t.update_materials(brighter(sc, factor))
            t.set_display(1, **kw)
            trace(t, W, H, 1)
            sync(t, W, H, 1, exposure=1.0)
            shown, info, acc = t.read_framebuffer(), t.read_exposure(), t.read_accumulator(1)
            t.set_display(0)
            sync(t, W, H, 1, exposure=1.0)
            out[name] = dict(shown=shown, plain=t.read_framebuffer(), info=info, acc=acc)
    finally:
        t.Close()
    base, x64 = out["base"], out["x64"]
    mean = lambda fb: float(fb[..., :3].mean())  # noqa: E731
    cpu_base = host.display(base["acc"], **kw)
    cpu_x64 = host.display(base["acc"] * F(64.0), **kw)
    band = abs(mean(cpu_x64[0]) - mean(cpu_base[0])) + 2.0
    print(f"\ndisplay x64: shown mean {mean(base['shown']):.2f} -> {mean(x64['shown']):.2f} (band {band:.2f}); plain mean {mean(base['plain']):.2f} -> "
          f"{mean(x64['plain']):.2f}; log2E {float(base['info']['log2E']):.4f} -> {float(x64['info']['log2E']):.4f}")
    assert np.array_equal(base["shown"], cpu_base[0])                           # (the frame on the device is the restatement's)
    assert abs(mean(x64["shown"]) - mean(base["shown"])) <= band
    assert abs((float(x64["info"]["log2E"]) - float(base["info"]["log2E"])) + 6.0) < 0.25   # six stops down
    grey = base["plain"][..., :3] >= 108
    assert grey.mean() > 0.02 and np.all(x64["plain"][..., :3][grey] >= 245)    # the plain frame saturates
    assert mean(x64["plain"]) - mean(base["plain"]) > 10 * band


# ---- 4. the exposure state -----------------------------------------------------------------------------------------------------------
def test_exposure_state_survives_camera_and_materials_and_is_reset_by_resize_and_set_display(built, host):
    from polaris_amd import scenes

    W = H = 48
    sc = scenes.cornell_box("layered")
    kw = dict(tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1, adapt=0.5)
    t = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        def frame(prev, W=W, H=H, **over):
            trace(t, W, H, 1)
            sync(t, W, H, 1, exposure=1.0)
            got = t.read_exposure()
            want = host.display(t.read_accumulator(1), prev_log2E=prev, **dict(kw, **over))
            assert same_info(got, want[2]) and np.array_equal(t.read_framebuffer(), want[0]), (prev, got, want[2])
            return got["log2E"]

        with pytest.raises(TracerError):
            t.read_exposure()                                                    # before any displayed sync
        sync_off = lambda: (trace(t, W, H, 1), sync(t, W, H, 1))  # noqa: E731
        sync_off()
        assert [t.kernel_ms(k)[1] for k in TIMERS] == [0, 0, 0, 1]              # off: the stage's kernels do not run
        with pytest.raises(TracerError):
            t.read_exposure()
        t.set_display(1, **kw)
        with pytest.raises(TracerError):
            t.read_exposure()                                                    # on, but nothing synced yet
        l0 = frame(None)                                                         # the first metered sync snaps
        moved = dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([0.4, 0.2, 0.0], F)).astype(F))
        t.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, moved)
        l1 = frame(l0)                                                           # a camera move: the state adapts from l0
        t.update_materials(brighter(sc, 64.0))
        l2 = frame(l1)                                                           # a material edit: from l1
        assert float(l2) < float(l1) - 2.0                                       # (half of six stops)
        t.set_display(1, **kw)                                                   # identical bytes: nothing happens
        assert bits(t.read_exposure()["log2E"]) == bits(l2)
        l3 = frame(l2)
        t.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc)          # an upload: the state stays
        l4 = frame(l3)
        t.set_display(1, **dict(kw, adapt=0.25))                                 # a changed byte: reset
        with pytest.raises(TracerError):
            t.read_exposure()
        l5 = frame(None, adapt=0.25)
        frame(l5, adapt=0.25)
        t.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (40, 32))   # a resize: reset
        with pytest.raises(TracerError):
            t.read_exposure()
        frame(None, W=40, H=32, adapt=0.25)
        t.set_display(0)                                                         # off, and on again: reset
        t.set_display(0, tone_operator=T.TONE_HABLE)                             # (any two off states are equal)
        with pytest.raises(TracerError):
            t.read_exposure()
        t.set_display(1, **kw)
        frame(None, W=40, H=32)
        assert l4 is not None
    finally:
        t.Close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_set_display_refusals_leave_the_state_unchanged(built, host):
    from polaris_amd import scenes

    W = H = 32
    kw = dict(tone_operator=T.TONE_HABLE, srgb=1, auto_exposure=1, adapt=0.5)
    t = make_hip_tracer(scenes.SCENES["cornell"](1.0), W, H)
    try:
        t.set_display(1, **kw)
        trace(t, W, H, 1)
        sync(t, W, H, 1, exposure=1.0)
        before, fb = t.read_exposure(), t.read_framebuffer()
        for bad in (dict(tone_operator=7), dict(srgb=3), dict(auto_exposure=2), dict(white=float("nan")), dict(white=1e9), dict(auto_exposure=1, key=0.0),
                    dict(auto_exposure=1, compensation_ev=99.0), dict(auto_exposure=1, low_permille=950, high_permille=500),
                    dict(auto_exposure=1, high_permille=2000), dict(auto_exposure=1, min_ev=3.0, max_ev=2.0), dict(auto_exposure=1, adapt=float("nan")),
                    dict(auto_exposure=1, adapt=2.0)):
            with pytest.raises(TracerError):
                t.set_display(1, **bad)
        for enabled in (2, 7):
            with pytest.raises(TracerError):
                t.set_display(enabled)
        p = T.display_params(1, **kw)
        p.struct_size += 4
        assert t._lib.polaris_hip_set_display(t._h, p) == 2 and t._lib.polaris_hip_set_display(t._h, None) == 2
        info = T.ExposureInfo()
        info.struct_size = 8
        assert t._lib.polaris_hip_read_exposure(t._h, info, None) == 2 and t._lib.polaris_hip_read_exposure(t._h, None, None) == 2
        after = t.read_exposure()                                                # the state and the params are what they were
        assert same_info(after, before) and np.array_equal(after["histogram"], before["histogram"])
        sync(t, W, H, 1, exposure=1.0)
        want = host.display(t.read_accumulator(1), prev_log2E=before["log2E"], **kw)
        assert same_info(t.read_exposure(), want[2]) and np.array_equal(t.read_framebuffer(), want[0])
        assert not np.array_equal(fb, want[0]) or float(before["log2E"]) == float(want[2]["log2E"])
    finally:
        t.Close()


# ---- 6. the host layer ---------------------------------------------------------------------------------------------------------------
def test_renderer_displays_and_reads_the_exposure_of_its_primary(built, host):
    """Three tracers with tracer 1 the primary: Renderer.set_display reaches every tracer, only the primary syncs, and read_exposure is
    the primary's -- the restatement of its frame accumulator, as the frame's bytes are.  A second frame adapts from the first."""
    from polaris_amd import scenes

    W, H, spp = 64, 60, 4
    kw = dict(tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1, adapt=0.5, compensation_ev=0.25)
    r = host.Renderer(scenes.SCENES["cornell"](W / H), [0, 0, 0], primary=1, width=W, height=H, spp=spp, exposure=1.2, seed=5)
    try:
        with pytest.raises(RuntimeError):
            r.read_exposure()                                                    # nothing displayed yet
        r.set_display(1, **kw)
        with pytest.raises(RuntimeError):
            r.set_display(1, tone_operator=9)
        prev = None
        for _ in range(2):
            r.render()
            fb, acc = r.read()
            got = r.read_exposure()
            want_fb, want_hist, want_info = host.display(acc, weight=F(1.0 / spp), exposure=1.2, prev_log2E=prev, **kw)
            assert same_info(got, want_info) and np.array_equal(got["histogram"], want_hist) and np.array_equal(fb, want_fb)
            assert got["valid"] == 1 and got["n_metered"] > W * H // 2
            prev = got["log2E"]
        r.set_display(0)
        with pytest.raises(RuntimeError):
            r.read_exposure()
        r.render()
        assert np.array_equal(r.read()[0], host.display(r.read()[1], weight=F(1.0 / spp), exposure=1.2)[0])   # off: the plain tone-map
    finally:
        r.close()


def test_render_py_writes_the_exposure_beside_the_frame(built, tmp_path):
    """render.py --tonemap aces --srgb --auto-exposure --aov-dir: the frame and exposure.json of its last metered sync."""
    import json
    import os

    from polaris_amd import render
    from test_gpu_denoise import ROOM_MTL, room_obj

    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    scene = str(tmp_path / "room.obj")
    out, aov = str(tmp_path / "frame.png"), str(tmp_path / "aov")
    assert render.main([scene, "--width", "48", "--height", "40", "--spp", "2", "--out", out, "--tonemap", "aces", "--srgb", "--auto-exposure",
                        "--ev-comp", "0.5", "--aov-dir", aov]) == 0
    e = json.load(open(os.path.join(aov, "exposure.json")))
    assert os.path.getsize(out) > 0 and e["valid"] == 1 and sum(e["histogram"]) == e["n_metered"] > 0 and abs(2.0 ** e["log2E"] - e["E"]) < 1e-4 * e["E"]
    plain = str(tmp_path / "plain.png")
    assert render.main([scene, "--width", "48", "--height", "40", "--spp", "2", "--out", plain]) == 0
    assert open(plain, "rb").read() != open(out, "rb").read()
    for bad in (["--white", "2.0"], ["--white", "2.0", "--tonemap", "aces"], ["--ev-comp", "1.0"], ["--adapt", "0.5", "--tonemap", "hable"]):
        with pytest.raises(SystemExit):                                          # flags that would be ignored are refused
            render.main([scene, "--out", plain] + bad)
