"""Temporal reuse across mesh deformation on the MI355X (include/polaris_hip.h: option "vertex_motion",
polaris_hip_reproject_deform_planes, polaris_hip_read_hit_plane).

Bars: k_reproject_deform<false> and <true> are bit-equal to the CPU restatement (polaris_host_reproject_deform) on the engineered
planes of tests/test_vertex_motion_cpu.py; the HIT plane is bit-equal to what the probe's traversal kernel and the CPU oracle return
for the pixel centres' rays; on the real path an update_vertices keeps the history, and the PRIOR, TEMPORAL and DENOISED planes and
the frame buffer are bit-equal to the host chain fed the device's own planes; two deformations without a sync in between reproject
from the older vertices; the option never changes an accumulator, a counter or the scene's allocations, and off or without effect
the update drops the history as it always did."""
import dataclasses

import numpy as np
import pytest

import gbuffer_oracle as G
import motion_oracle as MO
import vertex_motion_oracle as VO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

F = np.float32
TP = T.TEMPORAL_DEFAULTS
DN = T.DENOISE_DEFAULTS
VA = T.VARIANCE_DEFAULTS
W = H = 48
SPP = 2
ON = dict(object_motion=1, vertex_update=1, vertex_motion=1)


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


@pytest.fixture(scope="module")
def steps():
    """The two-instance Cornell box and two deformations of its tall block, built once: leave them unchanged."""
    base = VO.cornell_two_instances(W / H)
    return [base, VO.deformed_block(base, 1), VO.deformed_block(base, 2)]


def set_cam(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)


def deform(tr, sc):
    from polaris_amd import scenes

    vertices, boxes, _, _, ems = scenes.vertex_update_args(sc)
    tr.update_vertices(vertices, boxes, None, None, ems)


def moved_camera(sc):
    return dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([0.02, 0.01, 0], F)).astype(F))


# ---- 6. the kernel against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [TP, dict(max_history=4096, normal_threshold=-1.0, depth_threshold=1e6)])
def test_reproject_deform_planes_bit_equal_to_cpu(host, params):
    from polaris_amd.tracer import HipTracer

    tr = HipTracer("planes", 0)
    tr.Init()
    try:
        tr.set_option("time_kernels", 1)
        for name, c in VO.engineered_cases(32, 24):
            got = tr.reproject_deform_planes(*VO.args(c), **params)
            assert tr.kernel_symbol("reproject") == "pol::k_reproject_deform<false>"
            want = host.reproject_deform(*VO.args(c), **params)
            assert np.array_equal(bits(got), bits(want)), name
            got, got2 = tr.reproject_deform_planes(*VO.args(c), history_variance=c["hvar"], **params)
            assert tr.kernel_symbol("reproject") == "pol::k_reproject_deform<true>"
            want, want2 = host.reproject_deform(*VO.args(c), history_variance=c["hvar"], **params)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got2), bits(want2)), name + " (M2)"
            assert (want[..., 3] > 0).mean() > 0.25 and (want2[..., 0] > 0).mean() > 0.25, name
    finally:
        tr.Close()


# ---- 7. the HIT plane -----------------------------------------------------------------------------------------------------------
def test_hit_plane_is_the_probes_and_the_oracles_hit(oracle, steps):
    sc = steps[1]
    tr = make_hip_tracer(sc, W, H, **ON)
    try:
        tr.set_temporal()
        plane, inst, guide = tr.read_hit_plane(), tr.read_instance_plane(), tr.read_aov(T.AOV_GUIDE)
        rays = G.centre_rays(sc, W, H)
        hit, wuvt, tri = tr.probe_intersect(rays)
    finally:
        tr.Close()
    found = (np.asarray(hit) != 0).reshape(H, W)
    assert 0 < (~found).sum() < found.sum() or found.all()
    want = VO.hit_plane(np.where(found, np.asarray(tri).reshape(H, W), -1), wuvt[:, 1].reshape(H, W), wuvt[:, 2].reshape(H, W))
    assert np.array_equal(plane, want)
    assert np.array_equal(plane, VO.gbuffer_hit(oracle, sc, W, H)[3])
    assert np.all(plane[..., 3] == 0) and np.array_equal(plane[..., 0] == VO.NO_TRIANGLE, guide[..., 3] == G.FLT_MAX)
    assert {0, 1} <= set(np.unique(inst[found]).tolist()) and plane[found, 0].max() < len(sc.vertices) // 3


def test_hit_plane_misses(built):
    """A camera that looks past the box sees misses: 0xFFFFFFFF | 0 | 0 | 0 there, as the INSTANCE word."""
    sc = VO.cornell_two_instances(W / H)
    sc.set_camera(eye=(0.5, 0.5, -1.5), look=(1.2, 0.5, 0.5), fov=0.9, aspect=W / H)
    tr = make_hip_tracer(sc, W, H, **ON)
    try:
        tr.set_temporal()
        plane, inst = tr.read_hit_plane(), tr.read_instance_plane()
    finally:
        tr.Close()
    miss = inst == MO.NO_INSTANCE
    assert 0 < miss.sum() < miss.size
    assert np.all(plane[miss] == np.array([0xFFFFFFFF, 0, 0, 0], np.uint32)) and np.all(plane[~miss, 0] != VO.NO_TRIANGLE)


def test_hit_plane_of_a_chain_pixel_is_the_miss_word(built):
    sc = VO.cornell_two_instances(W / H, mirror=True)
    tr = make_hip_tracer(sc, W, H, guide_specular=2, **ON)
    try:
        tr.set_temporal()
        plane, inst, guide = tr.read_hit_plane(), tr.read_instance_plane(), tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    chain = (inst == MO.NO_INSTANCE) & (guide[..., 3] < G.FLT_MAX)
    assert chain.sum() > 20                                            # pixels that show the room in the mirror
    assert np.all(plane[inst == MO.NO_INSTANCE] == np.array([0xFFFFFFFF, 0, 0, 0], np.uint32))
    assert np.all(plane[inst != MO.NO_INSTANCE, 0] != VO.NO_TRIANGLE)


# ---- 8. the real path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variance", [False, True])
@pytest.mark.parametrize("move", [False, True])
def test_real_path_matches_host_chain(host, oracle, steps, move, variance):
    sc0, sc1 = steps[0], steps[1]
    cam1 = moved_camera(sc1) if move else sc1
    kw = dict(normal_power_log2=DN["normal_power_log2"], sigma_depth=DN["sigma_depth"], **VA)
    tr = make_hip_tracer(sc0, W, H, time_kernels=1, **ON)
    try:
        tr.set_denoise()
        tr.set_temporal()
        if variance:
            tr.set_variance(**VA)
        trace(tr, W, H, SPP, base=3)
        sync(tr, W, H, SPP)
        assert not tr.kernel_symbol("reproject").startswith("pol::k_reproject")      # (no history: the PRIOR was cleared)
        hist, g0, a0, i0 = tr.read_aov(T.AOV_TEMPORAL), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO), tr.read_instance_plane()
        hvar = tr.read_aov(T.AOV_VARIANCE) if variance else None
        counts = tr.scene_counts()
        deform(tr, sc1)                                    # (no camera call: the update alone turns the synced planes into the history)
        assert tr.scene_counts() == counts
        if move:
            set_cam(tr, cam1)
        trace(tr, W, H, SPP, base=5)
        sync(tr, W, H, SPP)
        assert tr.kernel_symbol("reproject") == f"pol::k_reproject_deform<{'true' if variance else 'false'}>"
        got = {k: tr.read_aov(k) for k in (T.AOV_PRIOR, T.AOV_TEMPORAL, T.AOV_DENOISED, T.AOV_GUIDE, T.AOV_ALBEDO)}
        if variance:
            got.update({k: tr.read_aov(k) for k in (T.AOV_PRIOR2, T.AOV_VARIANCE)})
        i1, h1 = tr.read_instance_plane(), tr.read_hit_plane()
        acc, fb = tr.read_accumulator(1), tr.read_framebuffer()
    finally:
        tr.Close()
    g1, a1 = got[T.AOV_GUIDE], got[T.AOV_ALBEDO]
    inv = MO.inv_table(sc0)
    args = (hist, g0, a0, i0, sc0.eye, sc0.frustum, g1, a1, i1, cam1.eye, cam1.frustum, inv, inv, h1, sc1.vertices, sc0.vertices)
    if variance:
        prior, prior2 = host.reproject_deform(*args, history_variance=hvar, **TP)
        assert np.array_equal(bits(got[T.AOV_PRIOR2]), bits(prior2)) and (prior2[..., 3] > 0).mean() > 0.5
    else:
        prior = host.reproject_deform(*args, **TP)
    block = G.filtered_mask(a1) & (i1 == 1)
    assert block.sum() > 100 and (prior[block, 3] > 0).mean() > 0.5 and (prior[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(got[T.AOV_PRIOR]), bits(prior))
    tmp = host.temporal_combine(acc, prior, 0, SPP)
    assert np.array_equal(bits(got[T.AOV_TEMPORAL]), bits(tmp))
    if variance:
        var = host.variance(acc, SPP, g1, a1, temporal=tmp, prior2=prior2, **kw)
        assert np.array_equal(bits(got[T.AOV_VARIANCE]), bits(var))
        den = host.denoise_variance(tmp, F(1), var, g1, a1, iterations=DN["iterations"], **kw)
    else:
        den = host.denoise(tmp, F(1), g1, a1, **DN)
    assert np.array_equal(bits(got[T.AOV_DENOISED][..., :3]), bits(den[..., :3]))
    assert np.array_equal(fb, oracle.tonemap(den, 1.0, 1.2).reshape(H, W, 4))
    # the rigid arithmetic looks at the same place for the deformed block: it differs from the PRIOR there
    rigid = host.reproject_motion(*args[:13], **TP)
    assert not np.array_equal(bits(rigid[block]), bits(prior[block]))
    room = G.filtered_mask(a1) & (i1 == 0)
    assert np.array_equal(bits(rigid[room]), bits(prior[room]))


def test_two_deformations_without_a_sync_reproject_from_the_older_vertices(host, steps):
    sc0, sc1, sc2 = steps
    tr = make_hip_tracer(sc0, W, H, time_kernels=1, **ON)
    try:
        tr.set_temporal()
        trace(tr, W, H, SPP, base=3)
        sync(tr, W, H, SPP)
        hist, g0, a0, i0 = tr.read_aov(T.AOV_TEMPORAL), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO), tr.read_instance_plane()
        deform(tr, sc1)
        trace(tr, W, H, SPP, base=4)                       # (a Trace, but no temporal sync, under the first deformation)
        deform(tr, sc2)
        trace(tr, W, H, SPP, base=5)
        sync(tr, W, H, SPP)
        assert tr.kernel_symbol("reproject") == "pol::k_reproject_deform<false>"
        prior, g2, a2, i2, h2 = tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO), tr.read_instance_plane(), tr.read_hit_plane()
    finally:
        tr.Close()
    inv = MO.inv_table(sc0)
    head = (hist, g0, a0, i0, sc0.eye, sc0.frustum, g2, a2, i2, sc2.eye, sc2.frustum, inv, inv, h2, sc2.vertices)
    want = host.reproject_deform(*head, sc0.vertices, **TP)
    assert (want[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(prior), bits(want))
    assert not np.array_equal(bits(prior), bits(host.reproject_deform(*head, sc1.vertices, **TP)))


# ---- 9. nothing else moves --------------------------------------------------------------------------------------------------------
def test_accumulators_counters_and_allocations_do_not_see_the_option(built, steps):
    sc0, sc1 = steps[0], steps[1]
    out = {}
    for name, opts in (("off", dict(object_motion=1, vertex_update=1)), ("on", ON), ("no vertex_update", dict(object_motion=1, vertex_motion=1))):
        tr = make_hip_tracer(sc0, W, H, samples_per_batch=2, time_kernels=1, **opts)
        try:
            tr.set_temporal()
            st0 = trace(tr, W, H, 4, base=3)
            sync(tr, W, H, 4)
            counts = tr.scene_counts()
            if name == "no vertex_update":
                with pytest.raises(RuntimeError):
                    deform(tr, sc1)                        # (refused as ever; and the option has no effect on this scene)
                with pytest.raises(RuntimeError):
                    tr.read_hit_plane()
                out[name] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st0), counts)
                continue
            deform(tr, sc1)
            st = trace(tr, W, H, 4, base=5)
            sync(tr, W, H, 4)
            out[name] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st0) + bytes(st), counts, tr.scene_counts(), tr.read_aov(T.AOV_PRIOR),
                         tr.kernel_symbol("reproject"), tr.kernel_symbol("gbuffer"))
        finally:
            tr.Close()
    off, on, plain = out["off"], out["on"], out["no vertex_update"]
    assert np.array_equal(bits(off[0]), bits(on[0])) and np.array_equal(bits(off[1]), bits(on[1]))
    n = len(off[2]) // 2
    assert off[2][:n - 8] == on[2][:n - 8] and off[2][n:-8] == on[2][n:-8]    # every counter (device_ms, the last field, is a time)
    assert plain[2][:n - 8] == on[2][:n - 8]
    assert off[3] == off[4] == on[3] == on[4]                                 # no additional scene allocation, before or after the update
    assert plain[3][:2] == on[3][:2] and plain[3][2] < on[3][2]              # (without vertex_update the upload keeps less)
    assert np.all(off[5] == 0)                                              # option off: the update dropped the history, m = 0 everywhere
    assert not off[6].startswith("pol::k_reproject")                        # ... and no reprojection kernel ran for it
    assert (on[5][..., 3] > 0).mean() > 0.5 and on[6] == "pol::k_reproject_deform<false>"
    assert off[7] == on[7] == "pol::k_gbuffer"


def test_kernel_symbol_names_the_deform_kernel_only_with_a_snapshot(built, steps):
    """Camera moves and instance moves with the option on go through k_reproject<*, true> as without it; the deform kernel runs only
    for a history whose vertices were overwritten, and no longer once a sync under the new vertices has become the history."""
    from polaris_amd import scenes

    sc0, sc1 = steps[0], steps[1]
    tr = make_hip_tracer(sc0, W, H, time_kernels=1, **ON)
    try:
        tr.set_temporal()
        trace(tr, W, H, SPP, base=3)
        sync(tr, W, H, SPP)
        set_cam(tr, moved_camera(sc0))
        trace(tr, W, H, SPP, base=4)
        sync(tr, W, H, SPP)
        assert tr.kernel_symbol("reproject") == "pol::k_reproject<false, true>"
        tr.update_instances(*scenes.instance_update_args(sc0))
        trace(tr, W, H, SPP, base=5)
        sync(tr, W, H, SPP)
        assert tr.kernel_symbol("reproject") == "pol::k_reproject<false, true>"
        deform(tr, sc1)
        trace(tr, W, H, SPP, base=6)
        sync(tr, W, H, SPP)
        assert tr.kernel_symbol("reproject") == "pol::k_reproject_deform<false>"
        set_cam(tr, sc1)                                   # the history is now the sync under the deformed vertices: nothing to undo
        trace(tr, W, H, SPP, base=7)
        sync(tr, W, H, SPP)
        assert tr.kernel_symbol("reproject") == "pol::k_reproject<false, true>"
        assert (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).mean() > 0.5
    finally:
        tr.Close()


@pytest.mark.parametrize("drop", ["materials", "toggle"])
def test_history_is_dropped(built, steps, drop):
    from polaris_amd import scenes

    sc0, sc1 = steps[0], steps[1]
    tr = make_hip_tracer(sc0, W, H, **ON)
    try:
        tr.set_temporal()
        trace(tr, W, H, SPP, base=3)
        sync(tr, W, H, SPP)
        deform(tr, sc1)
        if drop == "materials":
            tr.update_materials(*scenes.material_update_args(sc1))
        else:
            tr.set_option("vertex_motion", 0)
            with pytest.raises(RuntimeError):
                tr.read_hit_plane()
            tr.set_option("vertex_motion", 1)
        trace(tr, W, H, SPP, base=5)
        sync(tr, W, H, SPP)
        assert np.all(tr.read_aov(T.AOV_PRIOR) == 0)
        assert tr.read_hit_plane().shape == (H, W, 4)
    finally:
        tr.Close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_unchanged(host, steps):
    import ctypes as C

    from polaris_amd.tracer import TracerError

    sc0, sc1 = steps[0], steps[1]
    name, c = VO.engineered_cases(32, 24)[0]
    tr = make_hip_tracer(sc0, W, H, **ON)
    try:
        tr.set_temporal()
        trace(tr, W, H, SPP, base=3)
        sync(tr, W, H, SPP)
        deform(tr, sc1)
        trace(tr, W, H, SPP, base=5)
        sync(tr, W, H, SPP)
        before = (tr.read_aov(T.AOV_PRIOR), tr.read_hit_plane(), tr.read_framebuffer())
        assert (before[0][..., 3] > 0).mean() > 0.5

        def refused(call):
            with pytest.raises(TracerError) as e:
                call()
            assert e.value.code == 2, str(e.value)                         # POLARIS_E_BAD_ARGUMENT

        refused(lambda: tr.set_option("vertex_motion", 2))
        refused(lambda: tr.set_option("vertex_motion", -1))
        short = np.zeros(4 * W * H - 1, np.uint32)
        refused(lambda: tr._check(tr._lib.polaris_hip_read_hit_plane(tr._h, short.ctypes.data, short.size), tr._h))
        refused(lambda: tr._check(tr._lib.polaris_hip_read_hit_plane(tr._h, None, C.c_size_t(4 * W * H)), tr._h))
        a = VO.args(c)
        refused(lambda: tr.reproject_deform_planes(*a[:14], np.zeros((0, 4), F), np.zeros((0, 4), F), **TP))    # num_triangles = 0
        refused(lambda: tr.reproject_deform_planes(*a[:14], None, a[15], **TP))
        refused(lambda: tr.reproject_deform_planes(*a[:14], a[14], None, **TP))
        after = (tr.read_aov(T.AOV_PRIOR), tr.read_hit_plane(), tr.read_framebuffer())
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, after))
        tr.set_temporal(max_history=0)                                     # the option is no longer in effect
        refused(tr.read_hit_plane)
    finally:
        tr.Close()
    for opts in (dict(object_motion=1, vertex_update=1), dict(vertex_update=1, vertex_motion=1), dict(object_motion=1, vertex_motion=1)):
        tr = make_hip_tracer(sc0, W, H, **opts)                            # one of the three conditions is missing
        try:
            tr.set_temporal()
            with pytest.raises(TracerError) as e:
                tr.read_hit_plane()
            assert e.value.code == 2 and "vertex_motion" in str(e.value)
        finally:
            tr.Close()
