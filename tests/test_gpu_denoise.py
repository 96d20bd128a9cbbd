"""Denoising of the synced frame on the MI355X (include/polaris_hip.h: polaris_hip_set_denoise / polaris_hip_read_aov).

Bars: the G-buffer's hit distances and hit / miss pattern are bit-equal to the CPU oracle's closest hits of the restated
pixel-centre rays, its normals and albedo within 1e-5 of the oracle's material walk (untextured albedo exact); the DENOISED plane
is bit-equal to the CPU restatement (polaris_host_denoise) fed the device's own accumulator and G-buffer, and the frame buffer to
the oracle's tone-map of it; denoising never changes an accumulator or a counter."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import gbuffer_oracle as G
from conftest import ROOT, bits, make_hip_tracer
from polaris_amd import ctypes_api as T

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def weight_of(accumulated, spp):
    return F(1.0 / float(F(accumulated + spp)))   # (float)(1.0 / (float)(acc + spp)), as sync computes it


def trace(tr, W, H, spp, *, base=7, accumulated=0, bounces=5):
    from oracle import pybind as ob
    from polaris_amd import scenes

    req = ob.make_request(W, H, spp=spp, bounces=bounces, accumulated=accumulated)
    tr.Trace(req, scenes.make_seeds(spp, bounces, base=base))
    st = tr.last_trace_stats
    tr.MergeOutput(tr, req)        # the primary's own block into its frame accumulator (renderer/default.go:188-191)
    return st


def sync(tr, W, H, spp, *, accumulated=0, block_y=0, block_h=None, exposure=1.2):
    from oracle import pybind as ob

    tr.SyncFramebuffer(ob.make_request(W, H, spp=spp, accumulated=accumulated, block_y=block_y, block_h=block_h, exposure=exposure))


# ---- 1. G-buffer against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "transformed", "materials", "sphere"])
def test_gbuffer_matches_oracle(oracle, name):
    from polaris_amd import scenes

    W, H = 97, 61
    sc = scenes.SCENES[name](W / H)
    tr = make_hip_tracer(sc, W, H)
    try:
        guide, albedo = tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        tr.set_option("traversal", 0)              # the G-buffer is cached: the same planes whatever the options say
        again = tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    want_g, want_a, info = G.gbuffer(oracle, sc, W, H)
    assert np.array_equal(bits(again), bits(guide))
    hit = want_g[..., 3] < G.FLT_MAX
    assert hit.any() and (name != "sphere" or (~hit).any())
    assert np.array_equal(bits(guide[..., 3]), bits(want_g[..., 3]))                 # t and the hit / miss pattern, bit for bit
    assert np.array_equal(bits(albedo[..., 3]), bits(want_a[..., 3]))                 # the selected leaf
    np.testing.assert_allclose(guide[..., :3], want_g[..., :3], rtol=0, atol=1e-5)     # normal after bump / normal maps
    plain = ~info["textured"]
    assert np.array_equal(bits(albedo[plain]), bits(want_a[plain]))                   # untextured albedo (tint * k, clamped): exact
    np.testing.assert_allclose(albedo[..., :3], want_a[..., :3], rtol=0, atol=1e-5)   # textured: the oracle's texel sample
    if name == "materials":
        assert info["textured"].any()


def test_aov_errors(built):
    from polaris_amd import scenes
    from polaris_amd.tracer import ChangeType, ErrNoSceneData, HipTracer, TracerError, UpdateMode

    sc = scenes.SCENES["cornell-diffuse"]()
    tr = HipTracer("aov", 0)
    tr.Init()
    try:
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (16, 16))
        with pytest.raises(ErrNoSceneData):
            tr.read_aov(T.AOV_GUIDE)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc)
        with pytest.raises(TracerError) as e:
            tr.read_aov(T.AOV_ALBEDO)                                   # no camera
        assert e.value.code == 2
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)
        with pytest.raises(TracerError) as e:
            tr.read_aov(T.AOV_DENOISED)                                 # no denoised sync yet
        assert e.value.code == 2
        for bad in (dict(iterations=9), dict(normal_power_log2=11), dict(sigma_depth=-1.0), dict(sigma_luminance=float("inf"))):
            with pytest.raises(TracerError) as e:
                tr.set_denoise(**bad)
            assert e.value.code == 2
        assert tr.read_aov(T.AOV_GUIDE).shape == (16, 16, 4)
    finally:
        tr.Close()


# ---- 2. filter: GPU against CPU, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "materials"])
def test_filter_matches_cpu_restatement_bit_for_bit(host, oracle, name):
    from polaris_amd import scenes

    W, H, spp = 97, 61, 8
    sc = scenes.SCENES[name](W / H)
    tr = make_hip_tracer(sc, W, H)
    p = dict(iterations=5, normal_power_log2=7, sigma_depth=0.1, sigma_luminance=1.0)
    try:
        trace(tr, W, H, spp)
        sync(tr, W, H, spp)                                    # plain: the bytes a sub-block sync must leave alone
        fb_plain = tr.read_framebuffer()
        tr.set_denoise(**p)
        sync(tr, W, H, spp, block_y=17, block_h=23)            # sub-block
        den_sub, fb_sub = tr.read_aov(T.AOV_DENOISED), tr.read_framebuffer()
        sync(tr, W, H, spp)                                    # full frame
        den, fb = tr.read_aov(T.AOV_DENOISED), tr.read_framebuffer()
        acc, guide, albedo = tr.read_accumulator(1), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
    finally:
        tr.Close()
    w = weight_of(0, spp)
    want = host.denoise(acc, w, guide, albedo, **p)
    assert np.array_equal(bits(den[..., :3]), bits(want[..., :3]))
    assert np.array_equal(fb.reshape(-1, 4), oracle.tonemap(den, 1.0, 1.2))
    want_sub = host.denoise(acc, w, guide, albedo, block_y=17, block_h=23, **p)
    assert np.array_equal(bits(den_sub[17:40, :, :3]), bits(want_sub[17:40, :, :3]))
    assert np.array_equal(fb_sub[17:40].reshape(-1, 4), oracle.tonemap(den_sub[17:40], 1.0, 1.2))
    assert np.array_equal(fb_sub[:17], fb_plain[:17]) and np.array_equal(fb_sub[40:], fb_plain[40:])
    assert not np.array_equal(fb_sub[17:40], fb_plain[17:40])


# ---- 3. invariants ------------------------------------------------------------------------------------------------------------
def test_accumulators_and_counters_do_not_see_the_filter(built):
    from polaris_amd import scenes

    W, H = 80, 64
    sc = scenes.SCENES["cornell"](W / H)
    out = {}
    for on in (False, True):
        tr = make_hip_tracer(sc, W, H, samples_per_batch=4)
        try:
            if on:
                tr.set_denoise()
            st1 = trace(tr, W, H, 8, base=3)
            sync(tr, W, H, 8)
            st2 = trace(tr, W, H, 8, base=5, accumulated=8)
            sync(tr, W, H, 8, accumulated=8)
            fb_on = tr.read_framebuffer()
            tr.set_denoise(iterations=0)
            sync(tr, W, H, 8, accumulated=8)
            out[on] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st1), bytes(st2), tr.read_framebuffer(), fb_on)
        finally:
            tr.Close()
    off, on = out[False], out[True]
    assert np.array_equal(bits(off[0]), bits(on[0])) and np.array_equal(bits(off[1]), bits(on[1]))
    assert off[2][:-8] == on[2][:-8] and off[3][:-8] == on[3][:-8]     # every counter (device_ms, the last field, is a time)
    assert np.array_equal(off[4], on[4])                                 # iterations = 0 again: the plain tone-map bytes
    assert not np.array_equal(on[5], on[4])


# ---- 4. invalidation ----------------------------------------------------------------------------------------------------------
def test_gbuffer_follows_camera_scene_and_size(built):
    from polaris_amd import scenes
    from polaris_amd.tracer import ChangeType, UpdateMode

    W, H = 64, 48
    a = scenes.SCENES["cornell"](W / H)
    b = scenes.SCENES["cornell"](W / H)
    b.set_camera(eye=(0.3, 0.6, -1.2), look=(0.55, 0.4, 0.5), fov=0.8, aspect=W / H)
    c = scenes.SCENES["sphere"](W / H)
    c.eye, c.frustum = b.eye.copy(), b.frustum.copy()    # (a scene upload keeps the tracer's camera: b's)

    def fresh(sc, w, h):
        t = make_hip_tracer(sc, w, h)
        try:
            return t.read_aov(T.AOV_GUIDE), t.read_aov(T.AOV_ALBEDO)
        finally:
            t.Close()

    tr = make_hip_tracer(a, W, H)
    try:
        first = tr.read_aov(T.AOV_GUIDE)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, b)
        after_cam = tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, c)
        after_scene = tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (40, 30))
        after_size = tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
    finally:
        tr.Close()
    for got, want in ((after_cam, fresh(b, W, H)), (after_scene, fresh(c, W, H)), (after_size, fresh(c, 40, 30))):
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert not np.array_equal(bits(first), bits(after_cam[0]))


# ---- 5. frame loop and CLI ----------------------------------------------------------------------------------------------------
def test_renderer_frame_loop_denoises_on_the_primary(host, oracle):
    from polaris_amd import scenes

    W, H, spp = 72, 60, 4
    sc = scenes.SCENES["cornell"](W / H)
    r = host.Renderer(sc, [0, 0], width=W, height=H, spp=spp, seed=5)
    try:
        r.set_denoise()
        rows, _ = r.render()
        fb, acc = r.read()
        guide, albedo, den = r.read_aov(T.AOV_GUIDE), r.read_aov(T.AOV_ALBEDO), r.read_aov(T.AOV_DENOISED)
    finally:
        r.close()
    assert sum(rows) == H and len(rows) == 2
    want = host.denoise(acc, weight_of(0, spp), guide, albedo, **T.DENOISE_DEFAULTS)
    assert np.array_equal(bits(den[..., :3]), bits(want[..., :3]))
    assert np.array_equal(fb.reshape(-1, 4), oracle.tonemap(want, 1.0, 1.2))


ROOM_MTL = """newmtl white
Kd 0.725 0.71 0.68
newmtl red
Kd 0.63 0.065 0.05
newmtl green
Kd 0.14 0.45 0.091
newmtl light
Ke 17 12 4
"""


def room_obj():
    L = ["mtllib room.mtl", "camera_fov 0.69", "camera_eye 0 1 3.4", "camera_look 0 1 0", "camera_up 0 1 0", "o room"]
    quads = [("white", [(-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1)]), ("white", [(-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1)]),
             ("white", [(-1, 0, -1), (1, 0, -1), (1, 2, -1), (-1, 2, -1)]), ("red", [(-1, 0, 1), (-1, 0, -1), (-1, 2, -1), (-1, 2, 1)]),
             ("green", [(1, 0, -1), (1, 0, 1), (1, 2, 1), (1, 2, -1)]),
             ("light", [(-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (0.3, 1.98, 0.3), (-0.3, 1.98, 0.3)])]
    for mat, q in quads:
        L += [f"v {x} {y} {z}" for x, y, z in q]
    for i, (mat, _) in enumerate(quads):
        L += [f"usemtl {mat}", "f " + " ".join(str(4 * i + k + 1) for k in range(4))]
    return "\n".join(L) + "\n"


def read_png(path):
    """RGBA8 PNG (what renderer::WritePNG writes) -> (h, w, 4) uint8; all five row filters."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, b""
    w = h = 0
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert depth == 8 and ctype == 6
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    raw = zlib.decompress(idat)
    stride = 4 * w
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int32)
        cur = np.zeros(stride, np.int32)
        for x in range(stride):
            a = cur[x - 4] if x >= 4 else 0
            b = prev[x]
            c = prev[x - 4] if x >= 4 else 0
            if f == 0:
                pred = 0
            elif f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[x] = (line[x] + pred) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 4)


def test_render_cli_writes_denoised_frame_and_aov_images(host, tmp_path):
    from polaris_amd.tracer import ChangeType, HipTracer, UpdateMode

    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    W, H = 64, 48
    aov = tmp_path / "aov"
    cmd = [sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--width", str(W), "--height", str(H), "--spp", "4",
           "--denoise", "5", "--aov-dir", str(aov), "--out", str(tmp_path / "frame.png")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("frame.png", "aov/normals.png", "aov/depth.png", "aov/albedo.png"):
        assert os.path.getsize(tmp_path / name) > 0, name
    sc = host.read_scene(str(tmp_path / "room.obj"), aspect=W / H)
    tr = HipTracer("cli", 0)
    tr.Init()
    try:
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (W, H))
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)
        guide, albedo = tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
    finally:
        tr.Close()
    hit = guide[..., 3] < G.FLT_MAX
    assert hit.any()
    max_depth = max(F(1), guide[..., 3][hit].max())
    want_n = np.zeros((H, W, 4), np.uint8)
    want_d = np.zeros((H, W, 4), np.uint8)
    want_n[hit, :3] = ((guide[hit, :3] + F(1)) * F(255) * F(0.5)).astype(np.uint8)              # debug.cl: (uchar)((n + 1) * 255 * 0.5)
    want_d[hit, :3] = (F(255) * (F(1) - guide[hit, 3] / (max_depth + F(1)))).astype(np.uint8)[:, None]   # (uchar)(255 * (1 - t / (maxDepth + 1)))
    want_n[..., 3] = want_d[..., 3] = 255
    assert np.array_equal(read_png(aov / "normals.png"), want_n)
    assert np.array_equal(read_png(aov / "depth.png"), want_d)
    want_a = np.full((H, W, 4), 255, np.uint8)
    want_a[..., :3] = (albedo[..., :3] * F(255)).astype(np.uint8)
    assert np.array_equal(read_png(aov / "albedo.png"), want_a)


# ---- 6. quality on the device -------------------------------------------------------------------------------------------------
def test_quality_on_the_device(built):
    from polaris_amd import scenes

    N = 512
    sc = scenes.SCENES["cornell"]()
    tr = make_hip_tracer(sc, N, N)
    try:
        trace(tr, N, N, 256, base=99)
        ref = tr.read_accumulator(1)[..., :3] / 256
        tr.set_denoise()
        trace(tr, N, N, 4, base=11)
        sync(tr, N, N, 4)
        noisy = tr.read_accumulator(1)[..., :3] / 4
        den = tr.read_aov(T.AOV_DENOISED)[..., :3]
        guide = tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    rmse = lambda x, m=slice(None): float(np.sqrt(np.mean((x[m] - ref[m]) ** 2)))  # noqa: E731
    edges = G.edge_mask(guide)
    ratio, edge_ratio = rmse(den) / rmse(noisy), rmse(den, edges) / rmse(noisy, edges)
    print(f"denoised / noisy RMSE against 256 spp at {N}^2: {ratio:.3f} (edge pixels {edge_ratio:.3f})")
    assert ratio <= 0.6, ratio
    assert edge_ratio <= 1.0, edge_ratio
