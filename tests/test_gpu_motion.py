"""Temporal reuse across moving mesh instances on the MI355X (include/polaris_hip.h: option "object_motion",
polaris_hip_reproject_motion_planes, polaris_hip_read_instance_plane).

Bars: k_reproject<*, true> is bit-equal to the CPU restatement (polaris_host_reproject_motion) on engineered planes; on the real path an
upload that moves instances keeps the history, and the PRIOR, TEMPORAL and DENOISED planes and the frame buffer are bit-equal to the
host chain fed the planes read before and after the upload; the INSTANCE plane names the instance whose mesh box holds the first hit;
the option never changes an accumulator or a counter, and with it off, after an incompatible upload or after a toggle the history is
dropped."""
import dataclasses

import numpy as np
import pytest

import gbuffer_oracle as G
import motion_oracle as MO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

F = np.float32
TP = T.TEMPORAL_DEFAULTS


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def upload(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc)


def set_cam(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)


# ---- 1. the test entry against the CPU restatement ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return [(f"{name} {W}x{H}", c) for W, H in ((64, 64), (97, 61)) for name, c in MO.engineered_cases(W, H)]


@pytest.mark.parametrize("params", [TP, dict(max_history=4, normal_threshold=0.5, depth_threshold=0.3),
                                    dict(max_history=4096, normal_threshold=-1.0, depth_threshold=1e6)])
def test_reproject_motion_planes_bit_equal_to_cpu(host, cases, params):
    from polaris_amd.tracer import HipTracer

    tr = HipTracer("planes", 0)
    tr.Init()
    try:
        for name, c in cases:
            got = tr.reproject_motion_planes(*MO.args(c), **params)
            want = host.reproject_motion(*MO.args(c), **params)
            assert np.array_equal(bits(got), bits(want)), name
            got, got2 = tr.reproject_motion_planes(*MO.args(c), history_variance=c["hvar"], **params)
            want, want2 = host.reproject_motion(*MO.args(c), history_variance=c["hvar"], **params)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got2), bits(want2)), name + " (M2)"
            if not name.startswith(("invalid", "instance mismatch")):
                assert (want[c["i"] == 1, 3] > 0).mean() > 0.3, name     # (the box's pixels do find history through the motion table)
    finally:
        tr.Close()


# ---- 2. the real path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,move", [((0, None), False), ((13, 21), False), ((0, None), True)])
def test_real_path_matches_host_chain(host, oracle, block, move):
    from polaris_amd import scenes

    W, H, spp = 96, 72, 4
    by, bh = block
    rows = slice(by, H if bh is None else by + bh)
    sc0, sc1 = scenes.moving_instances(0, W / H), scenes.moving_instances(1, W / H)
    cam1 = dataclasses.replace(sc1, eye=(np.asarray(sc1.eye, F) + np.array([0.02, 0.01, 0], F)).astype(F)) if move else sc1
    tr = make_hip_tracer(sc0, W, H, object_motion=1)
    try:
        tr.set_denoise()
        tr.set_temporal()
        trace(tr, W, H, spp, base=3)
        sync(tr, W, H, spp)
        hist, g0, a0, i0 = tr.read_aov(T.AOV_TEMPORAL), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO), tr.read_instance_plane()
        upload(tr, sc1)                                    # (no camera call: the upload alone turns the synced planes into the history)
        if move:
            set_cam(tr, cam1)
        fb_before = tr.read_framebuffer()
        trace(tr, W, H, spp, base=5)
        sync(tr, W, H, spp, block_y=by, block_h=bh)
        got = {k: tr.read_aov(k) for k in (T.AOV_PRIOR, T.AOV_TEMPORAL, T.AOV_DENOISED, T.AOV_GUIDE, T.AOV_ALBEDO)}
        i1 = tr.read_instance_plane()
        acc, fb = tr.read_accumulator(1), tr.read_framebuffer()
    finally:
        tr.Close()
    g1, a1 = got[T.AOV_GUIDE], got[T.AOV_ALBEDO]
    prior = host.reproject_motion(hist, g0, a0, i0, sc0.eye, sc0.frustum, g1, a1, i1, cam1.eye, cam1.frustum, MO.inv_table(sc0), MO.inv_table(sc1), **TP)
    tmp = host.temporal_combine(acc, prior, 0, spp, block_y=by, block_h=bh)
    den = host.denoise(tmp, F(1), g1, a1, block_y=by, block_h=bh, **T.DENOISE_DEFAULTS)
    moved = G.filtered_mask(a1) & ((i1 == 1) | (i1 == 2))
    assert moved.sum() > 200 and (prior[moved, 3] > 0).mean() > 0.5
    assert (prior[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(got[T.AOV_PRIOR]), bits(prior))
    assert np.array_equal(bits(got[T.AOV_TEMPORAL][rows]), bits(tmp[rows]))
    assert np.all(got[T.AOV_TEMPORAL][:by, :, 3] == 0)                            # (cleared at the first sync after the upload)
    assert np.array_equal(bits(got[T.AOV_DENOISED][rows, :, :3]), bits(den[rows, :, :3]))
    want_fb = oracle.tonemap(den, 1.0, 1.2).reshape(H, W, 4)
    assert np.array_equal(fb[rows], want_fb[rows])
    outside = np.ones(H, bool)
    outside[rows] = False
    assert np.array_equal(fb[outside], fb_before[outside])                         # rows outside the request keep their bytes
    # the camera-only arithmetic would have ghosted: it differs from the PRIOR on the moved instances
    plain = host.reproject(hist, g0, a0, sc0.eye, sc0.frustum, g1, a1, cam1.eye, cam1.frustum, **TP)
    assert not np.array_equal(bits(plain[moved]), bits(prior[moved]))


# ---- 3. the INSTANCE plane ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cubes", "transformed", "cornell"])
def test_instance_plane_is_geometrically_right(built, name):
    """Every hit pixel's first hit, taken to the mesh space of the instance the plane names, lies inside that mesh's root box (inflated
    by 1e-4 of its diagonal); with disjoint instances no other instance's matrix puts it there.  cornell: one instance, the
    root_is_instance path of the traversal."""
    from polaris_amd import scenes
    import temporal_oracle as TO

    W, H = 97, 61
    sc = scenes.SCENES[name](W / H)
    tr = make_hip_tracer(sc, W, H, object_motion=1)
    try:
        tr.set_temporal()
        inst, guide = tr.read_instance_plane(), tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    miss = guide[..., 3] == G.FLT_MAX
    assert np.array_equal(inst == MO.NO_INSTANCE, miss)
    hit = ~miss
    n = len(sc.mesh_instances)
    assert hit.any() and inst[hit].max() < n and (name == "cornell" or len(np.unique(inst[hit])) >= 4)
    p = np.asarray(sc.eye, np.float64) + guide[..., 3:4].astype(np.float64) * TO.centre_dirs(sc.eye, sc.frustum, W, H)
    for k in np.unique(inst[hit]):
        m = inst == k
        M = MO.mat4(sc.mesh_instances[k]["inv_transform"])
        q = p[m] @ M[:3, :3].T + M[:3, 3]
        root = sc.bvh_nodes[int(sc.mesh_instances[k]["bvh_root"])]
        lo, hi = root["min"].astype(np.float64), root["max"].astype(np.float64)
        tol = 1e-4 * np.linalg.norm(hi - lo)
        assert np.all((q >= lo - tol) & (q <= hi + tol)), (name, int(k))


# ---- 4. invariants ------------------------------------------------------------------------------------------------------------
def test_accumulators_and_counters_do_not_see_the_option(built):
    from polaris_amd import scenes

    W, H = 80, 64
    sc0, sc1 = scenes.moving_instances(0, W / H), scenes.moving_instances(1, W / H)
    out = {}
    for on in (0, 1):
        tr = make_hip_tracer(sc0, W, H, samples_per_batch=4, object_motion=on)
        try:
            tr.set_temporal()
            st0 = trace(tr, W, H, 16, base=3)
            sync(tr, W, H, 16)
            upload(tr, sc1)
            st = trace(tr, W, H, 16, base=5)
            sync(tr, W, H, 16)
            out[on] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st0) + bytes(st), tr.read_framebuffer(), tr.read_aov(T.AOV_PRIOR))
        finally:
            tr.Close()
    off, on = out[0], out[1]
    assert np.array_equal(bits(off[0]), bits(on[0])) and np.array_equal(bits(off[1]), bits(on[1]))
    n = len(off[2]) // 2
    assert off[2][:n - 8] == on[2][:n - 8] and off[2][n:-8] == on[2][n:-8]    # every counter (device_ms, the last field, is a time)
    assert np.all(off[4] == 0)                                              # option off: the upload dropped the history
    assert (on[4][..., 3] > 0).mean() > 0.5 and not np.array_equal(off[3], on[3])


@pytest.mark.parametrize("drop", ["incompatible", "toggle", "max_history", "resize"])
def test_history_is_dropped(built, drop):
    from polaris_amd import scenes
    from polaris_amd.tracer import ChangeType, UpdateMode

    W, H = 64, 48
    first = scenes.instanced_cubes(3, W / H) if drop == "incompatible" else scenes.moving_instances(0, W / H)
    second = scenes.instanced_cubes(2, W / H) if drop == "incompatible" else scenes.moving_instances(1, W / H)
    tr = make_hip_tracer(first, W, H, object_motion=1)
    try:
        tr.set_temporal()
        trace(tr, W, H, 4)
        sync(tr, W, H, 4)
        if drop != "incompatible":                    # (a compatible upload does keep it)
            upload(tr, second)
            trace(tr, W, H, 4, base=8)
            sync(tr, W, H, 4)
            assert (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
        if drop == "toggle":
            tr.set_option("object_motion", 0)
            with pytest.raises(RuntimeError):
                tr.read_instance_plane()
            tr.set_option("object_motion", 1)
        elif drop == "max_history":
            tr.set_temporal(max_history=0)
            with pytest.raises(RuntimeError):
                tr.read_instance_plane()                # (the option has an effect only with temporal reuse on)
            tr.set_temporal()
        elif drop == "resize":
            W, H = 48, 40
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (W, H))
        if drop == "incompatible":
            upload(tr, second)
        set_cam(tr, second)
        trace(tr, W, H, 4, base=9)
        sync(tr, W, H, 4)
        assert np.all(tr.read_aov(T.AOV_PRIOR) == 0)
        assert tr.read_instance_plane().shape == (H, W)
    finally:
        tr.Close()


def test_read_instance_plane_refuses_with_the_option_off(built):
    from polaris_amd import scenes
    from polaris_amd.tracer import TracerError

    W, H = 32, 24
    tr = make_hip_tracer(scenes.moving_instances(0, W / H), W, H)
    try:
        tr.set_temporal()
        with pytest.raises(TracerError) as e:
            tr.read_instance_plane()
        assert e.value.code == 2 and "object_motion" in str(e.value)               # POLARIS_E_BAD_ARGUMENT
        with pytest.raises(TracerError):
            tr.set_option("object_motion", 2)
        tr.set_option("object_motion", 1)
        assert set(np.unique(tr.read_instance_plane()).tolist()) <= {0, 1, 2, int(MO.NO_INSTANCE)}
    finally:
        tr.Close()


def test_option_set_after_the_scene(built):
    """Turned on after the upload, the option takes the matrices from the uploaded instance records: a camera move reuses the history
    at once; the first upload after it still drops the history (the old scene's mesh indices were not kept), the next one keeps it."""
    from polaris_amd import scenes

    W, H = 64, 48
    sc = [scenes.moving_instances(k, W / H) for k in range(3)]
    cam = dataclasses.replace(sc[0], eye=(np.asarray(sc[0].eye, F) + np.array([0.02, 0, 0], F)).astype(F))
    tr = make_hip_tracer(sc[0], W, H)
    try:
        tr.set_temporal()
        tr.set_option("object_motion", 1)
        trace(tr, W, H, 4)
        sync(tr, W, H, 4)
        inst = tr.read_instance_plane()
        assert {0, 1, 2} <= set(np.unique(inst).tolist()) <= {0, 1, 2, int(MO.NO_INSTANCE)}
        set_cam(tr, cam)
        trace(tr, W, H, 4, base=8)
        sync(tr, W, H, 4)
        assert (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
        upload(tr, sc[1])
        trace(tr, W, H, 4, base=9)
        sync(tr, W, H, 4)
        assert np.all(tr.read_aov(T.AOV_PRIOR) == 0)
        upload(tr, sc[2])
        trace(tr, W, H, 4, base=10)
        sync(tr, W, H, 4)
        prior, inst = tr.read_aov(T.AOV_PRIOR), tr.read_instance_plane()
        assert (prior[..., 3] > 0).mean() > 0.5 and (prior[(inst == 1) | (inst == 2), 3] > 0).mean() > 0.5
    finally:
        tr.Close()


def test_renderer_set_object_motion_reaches_the_primary(host):
    """Renderer.set_object_motion: the toggle drops the primary's history (the next move finds none), and with it on the camera moves
    of the frame loop go through the motion kernel and give the PRIOR of the camera-only reprojection (one STATIC instance)."""
    from polaris_amd import scenes

    W, H, spp = 72, 60, 4
    sc0 = scenes.SCENES["cornell"](W / H)         # (one instance: every INSTANCE word is 0, so the two arithmetics agree bit for bit)
    cams = [dataclasses.replace(sc0, eye=(np.asarray(sc0.eye, F) + np.array([0.02 * k, 0, 0], F)).astype(F)) for k in range(4)]
    r = host.Renderer(sc0, [0, 0], width=W, height=H, spp=spp, seed=5)
    try:
        r.set_temporal()
        r.render()
        r.set_camera(cams[1].eye, cams[1].frustum)
        r.render()
        assert (r.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
        r.set_object_motion(True)
        r.set_camera(cams[2].eye, cams[2].frustum)
        r.render()
        assert np.all(r.read_aov(T.AOV_PRIOR) == 0)                 # (the toggle dropped the history)
        hist, g0, a0 = r.read_aov(T.AOV_TEMPORAL), r.read_aov(T.AOV_GUIDE), r.read_aov(T.AOV_ALBEDO)
        r.set_camera(cams[3].eye, cams[3].frustum)
        r.render()
        prior, g1, a1 = r.read_aov(T.AOV_PRIOR), r.read_aov(T.AOV_GUIDE), r.read_aov(T.AOV_ALBEDO)
        with pytest.raises(RuntimeError):
            r.set_option("object_motion", 2)
        r.set_object_motion(False)
    finally:
        r.close()
    want = host.reproject(hist, g0, a0, cams[2].eye, cams[2].frustum, g1, a1, cams[3].eye, cams[3].frustum, **TP)
    assert (want[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(prior), bits(want))
