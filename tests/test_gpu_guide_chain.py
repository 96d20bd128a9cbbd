"""The tracer option "guide_specular" on the MI355X (include/polaris_hip.h).

Bars: off is off (k_gbuffer, every plane, accumulator, counter and frame-buffer byte); with N > 0 the planes' hit distances, leaf
words and INSTANCE words are bit-equal to the CPU restatement (tests/guide_chain_oracle.py), normals and albedo within 1e-5 of it
(untextured albedo exact); the planes are cached and a change of N recomputes them and drops the temporal history; reprojection
through the planar mirror finds the history; the DENOISED plane is bit-equal to polaris_host_denoise fed the chained planes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gbuffer_oracle as G
import guide_chain_oracle as GC
import temporal_oracle as TO
import test_guide_chain_cpu as TC
from conftest import ROOT, bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_denoise import ROOM_MTL, read_png, room_obj, sync, trace, weight_of
from test_gpu_temporal import set_cam

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 97, 61
TP = T.TEMPORAL_DEFAULTS


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def scene(name):
    from polaris_amd import scenes

    return TC.room(W / H) if name == "mirror_room" else scenes.SCENES[name](W / H)


def planes(tr):
    return tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def with_motion(tr):
    """(guide, albedo, INSTANCE) with object motion in effect."""
    tr.set_option("object_motion", 1)
    tr.set_temporal()
    return planes(tr) + (tr.read_instance_plane(),)


# ---- 1. off is off --------------------------------------------------------------------------------------------------------------
def test_off_is_off(built):
    sc = scene("mirror_room")
    out = {}
    for mode in ("fresh", "never", "back"):                      # a fresh tracer told 0 | never told | told 4, then 0
        tr = make_hip_tracer(sc, W, H, time_kernels=1)               # (the timers note the symbol they bracket)
        try:
            if mode == "fresh":
                tr.set_option("guide_specular", 0)
            if mode == "back":
                tr.set_option("guide_specular", 4)
                chained = planes(tr)
                assert tr.kernel_symbol("gbuffer") == "pol::k_gbuffer_chain"
                tr.set_option("guide_specular", 0)
            out[mode] = with_motion(tr)
            assert tr.kernel_symbol("gbuffer") == "pol::k_gbuffer"
        finally:
            tr.Close()
    assert same(out["fresh"], out["never"]) and same(out["fresh"], out["back"])
    assert not np.array_equal(bits(chained[0]), bits(out["fresh"][0]))


def test_accumulators_counters_and_frame_bytes_do_not_see_the_option(built):
    sc = scene("mirror_room")
    out = {}
    for links in (0, 4):
        tr = make_hip_tracer(sc, W, H, guide_specular=links)
        try:
            st = trace(tr, W, H, 4, base=3)
            sync(tr, W, H, 4)
            planes(tr)                                           # (the G-buffer is computed; nothing else may notice)
            sync(tr, W, H, 4)
            out[links] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st), tr.read_framebuffer())
        finally:
            tr.Close()
    a, b = out[0], out[4]
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert a[2][:-8] == b[2][:-8]                                # every counter (device_ms, the last field, is a time)
    assert np.array_equal(a[3], b[3])


# ---- 2. device = restatement ------------------------------------------------------------------------------------------------------
CASES = [(n, k) for n in ("mirror_room", "cornell") for k in (1, 2, 4, 8)] + [("transformed", 4)]


@pytest.mark.parametrize("name,links", CASES)
def test_planes_match_the_restatement(oracle, name, links):
    sc = scene(name)
    tr = make_hip_tracer(sc, W, H, guide_specular=links)
    try:
        guide, albedo = planes(tr)
        m_guide, m_albedo, inst = with_motion(tr)
    finally:
        tr.Close()
    want_g, want_a, want_i, info = TC.chained(oracle, sc, W, H, links)
    assert same((guide, albedo), (m_guide, m_albedo))
    assert np.array_equal(bits(guide[..., 3]), bits(want_g[..., 3]))                 # T and the hit / miss pattern, bit for bit
    assert np.array_equal(bits(albedo[..., 3]), bits(want_a[..., 3]))                 # the final leaf
    assert np.array_equal(inst, want_i)
    np.testing.assert_allclose(guide[..., :3], want_g[..., :3], rtol=0, atol=1e-5)
    plain = ~info["textured"]
    assert np.array_equal(bits(albedo[plain]), bits(want_a[plain]))
    np.testing.assert_allclose(albedo[..., :3], want_a[..., :3], rtol=0, atol=1e-5)
    if name == "transformed":   # scaled and rotated instances; its balls are mix(diffuse, conductor): the walk picks the mirror on some pixels
        assert len(np.unique(inst[info["k"] == 0])) >= 5 and (info["k"] >= 1).sum() > 30
        assert np.all(inst[info["k"] >= 1] == GC.NO_INSTANCE)
    else:
        assert (info["k"] >= 1).sum() > 100 and info["k"].max() == links


# ---- 3. cached, invalidated -------------------------------------------------------------------------------------------------------
def test_cached_and_invalidated(built):
    from polaris_amd.tracer import TracerError

    sc0 = scene("mirror_room")
    sc1 = TC.room(W / H, TC.SHIFT)
    fresh = {}
    for links in (2, 4):
        t = make_hip_tracer(sc1, W, H, guide_specular=links)
        try:
            fresh[links] = planes(t)
        finally:
            t.Close()
    tr = make_hip_tracer(sc0, W, H, guide_specular=2)
    try:
        tr.set_temporal()
        trace(tr, W, H, 2, base=3)
        sync(tr, W, H, 2)
        set_cam(tr, sc1)
        first = planes(tr)
        tr.set_option("traversal", 0)
        tr.set_option("node_mode", 0)
        assert same(planes(tr), first) and same(first, fresh[2])     # cached: the options do not reach the planes
        trace(tr, W, H, 2, base=5)
        sync(tr, W, H, 2)
        assert (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
        tr.set_option("guide_specular", 2)                          # the same value: nothing happens
        assert (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
        tr.set_option("guide_specular", 4)
        with pytest.raises(TracerError) as e:
            tr.read_aov(T.AOV_PRIOR)                                 # the history went with the old guide
        assert e.value.code == 2
        assert same(planes(tr), fresh[4]) and not same(fresh[4], fresh[2])
        sync(tr, W, H, 2)
        assert np.all(tr.read_aov(T.AOV_PRIOR)[..., 3] == 0)
    finally:
        tr.Close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_values_outside_0_to_8_are_refused(built):
    from polaris_amd.tracer import TracerError

    tr = make_hip_tracer(scene("mirror_room"), W, H, guide_specular=2)
    try:
        before = planes(tr)
        for bad in (-1, 9):
            with pytest.raises(TracerError) as e:
                tr.set_option("guide_specular", bad)
            assert e.value.code == 2
        assert same(planes(tr), before)
        tr.set_option("guide_specular", 8)
        assert not same(planes(tr), before)
    finally:
        tr.Close()


# ---- 5. reprojection end to end -----------------------------------------------------------------------------------------------------
def test_reprojection_through_the_planar_mirror_on_the_device(host, oracle):
    """The experiment of test_guide_chain_cpu.py through the device: its two cameras, its frame, N = 2."""
    RW, RH = TC.RW, TC.RH
    a, b = TC.room(RW / RH, 0.0, TC.RFOV), TC.room(RW / RH, TC.SHIFT, TC.RFOV)
    tr = make_hip_tracer(a, RW, RH, guide_specular=2)
    try:
        tr.set_temporal()
        trace(tr, RW, RH, 4, base=3)
        sync(tr, RW, RH, 4)
        hist, g0, a0 = (tr.read_aov(T.AOV_TEMPORAL),) + planes(tr)
        set_cam(tr, b)
        trace(tr, RW, RH, 4, base=5)
        sync(tr, RW, RH, 4)
        prior, (g1, a1) = tr.read_aov(T.AOV_PRIOR), planes(tr)
    finally:
        tr.Close()
    want_g, want_a, _, info = TC.chained(oracle, b, RW, RH, 2)
    assert np.array_equal(bits(g1[..., 3]), bits(want_g[..., 3])) and np.array_equal(bits(a1[..., 3]), bits(want_a[..., 3]))
    elig = GC.reprojection_eligible(b, g1, a1, info)
    assert elig.sum() > 0.5 * RW * RH
    share = float((prior[..., 3][elig] > 0).mean())
    print("eligible", int(elig.sum()), "with history", share)
    assert share >= 0.9
    # the comparison of tests/test_gpu_temporal.py: the CPU restatement fed the device's own planes, bit for bit
    assert np.array_equal(bits(prior), bits(host.reproject(hist, g0, a0, a.eye, a.frustum, g1, a1, b.eye, b.frustum, **TP)))
    # and the independent numpy statement over the experiment's pixels.  (Its margin cannot pick pixels here: a sideways move keeps
    # every point on its pixel row, the vertical bilinear fraction is 0 and so is the margin; the eligible pixels are away from every
    # G-buffer edge instead.)  float32 places a projected point within ~1e-4 pixel (tests/test_temporal_cpu.py), so a bilinear mean
    # moves by up to 2e-4 of the range of its taps per axis: 4e-4 of the largest history value bounds that for this noisy history.
    want, _ = TO.reproject(hist, g0, a0, a.eye, a.frustum, g1, a1, b.eye, b.frustum, **TP)
    top = float(np.max(hist[..., :3][np.isfinite(hist[..., :3])]))
    np.testing.assert_allclose(prior[elig], want[elig], rtol=1e-5, atol=1e-5 + 4e-4 * top)


# ---- 6. filter end to end -----------------------------------------------------------------------------------------------------------
def test_denoised_is_the_cpu_filter_of_the_chained_planes(host):
    spp = 4
    tr = make_hip_tracer(scene("mirror_room"), W, H, guide_specular=4)
    try:
        tr.set_denoise(iterations=4)
        trace(tr, W, H, spp)
        sync(tr, W, H, spp)
        den, acc, (guide, albedo) = tr.read_aov(T.AOV_DENOISED), tr.read_accumulator(1), planes(tr)
    finally:
        tr.Close()
    assert (G.edge_mask(guide) & (GC.leaf_types(albedo) == T.BXDF_DIFFUSE)).any()
    want = host.denoise(acc, weight_of(0, spp), guide, albedo, **dict(T.DENOISE_DEFAULTS, iterations=4))
    assert np.array_equal(bits(den[..., :3]), bits(want[..., :3]))


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------
MIRROR_MTL = ROOM_MTL + "newmtl mirror\nmat_expr conductor(specularity:{0.9,0.9,0.95})\n"


def mirror_room_obj():
    """test_gpu_denoise's room with an upright mirror turned 45 degrees: it shows the x = 1 wall, nearer than the room's far corners
    (so depth.png's normalisation, the largest distance of the frame, is the same with and without the flag)."""
    q = [(0.0, 0.5, 0.3), (0.6, 0.5, -0.3), (0.6, 1.5, -0.3), (0.0, 1.5, 0.3)]
    return room_obj() + "".join(f"v {x} {y} {z}\n" for x, y, z in q) + "usemtl mirror\nf 25 26 27 28\n"


def test_render_cli_follows_the_mirror_in_the_aov_images(host, tmp_path):
    from polaris_amd.tracer import ChangeType, HipTracer, UpdateMode

    (tmp_path / "room.obj").write_text(mirror_room_obj())
    (tmp_path / "room.mtl").write_text(MIRROR_MTL)
    Wc, Hc = 64, 48
    imgs = {}
    for links in (0, 2):
        aov = tmp_path / f"aov{links}"
        cmd = [sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--width", str(Wc), "--height", str(Hc), "--spp", "1",
               "--aov-dir", str(aov), "--out", str(tmp_path / f"frame{links}.png")] + (["--guide-specular", str(links)] if links else [])
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        imgs[links] = {n: read_png(aov / f"{n}.png") for n in ("normals", "depth", "albedo")}
    sc = host.read_scene(str(tmp_path / "room.obj"), aspect=Wc / Hc)
    tr = HipTracer("cli", 0)
    tr.Init()
    try:
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (Wc, Hc))
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)
        mirror = GC.leaf_types(tr.read_aov(T.AOV_ALBEDO)) == T.BXDF_CONDUCTOR
    finally:
        tr.Close()
    assert 50 < mirror.sum() < Wc * Hc / 4
    for n in ("normals", "depth", "albedo"):
        differs = np.any(imgs[0][n] != imgs[2][n], axis=-1)
        assert not differs[~mirror].any(), n
        assert differs[mirror].any(), n
    assert np.any(imgs[0]["normals"] != imgs[2]["normals"], axis=-1)[mirror].all()   # the wall's normal in the mirror's place
    assert os.path.getsize(tmp_path / "frame2.png") > 0
