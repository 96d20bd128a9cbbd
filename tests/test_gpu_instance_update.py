"""Moving mesh instances in place on the MI355X (polaris_hip_update_instances, option "instance_update").

Set-up: tracer A uploads `base` with the option on and calls update_instances with `moved`'s matrices, boxes and emissives; tracer B
uploads scenes.refit_instances(base, moved), the scene the update is defined to equal.  Bars: the device's pair and instance records
of A and B are byte-equal (with leaf subdivision on: up to the order of a tiny scene's triangle slots, tests/test_instance_update_cpu.py);
frames, probes and taps of A, of B and of the CPU oracle on the refit arrays are bit-equal, whatever traversal kernel runs; the temporal
history is treated as by an upload_scene; with the option off nothing changes, nothing is allocated, and the call is refused; a
refused call leaves the next frame bit-equal to the frame before it.
"""
import ctypes as C

import numpy as np
import pytest

import instance_update_cases as cases
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from polaris_amd import scenes
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

W, H, SPP, B = 64, 48, 2, 3
E_BAD_ARGUMENT, E_BAD_SCENE, E_UNSUPPORTED = 2, 5, 6


def upload(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc)


def updated(base, moved, **options):
    tr = make_hip_tracer(base, W, H, instance_update=1, **options)
    tr.update_instances(*scenes.instance_update_args(moved))
    return tr


def counters(st):
    return (list(st.rays_per_bounce[:B]), list(st.occl_per_bounce[:B]), st.primary_rays, st.indirect_rays, st.occlusion_rays,
            st.shaded_hits, st.shaded_misses, st.emitter_hits, st.unoccluded)


def frame(tr, base=21):
    """(trace accumulator, counters) of one frame."""
    from oracle import pybind as ob

    tr.Trace(ob.make_request(W, H, spp=SPP, bounces=B), scenes.make_seeds(SPP, B, base=base))
    return tr.read_accumulator(0), counters(tr.last_trace_stats)


def same_records(a, b, exact):
    """Pair and instance records of two tracers.  exact: every byte.  Else -- only a scene of at most 2 046 triangles with leaf
    subdivision on, whose slot order follows the padding (tests/test_instance_update_cpu.py, which resolves the references; the tap
    here does not read triangle records) -- every byte but the slot a triangle-leaf reference names."""
    (pa, ia), (pb, ib) = a, b
    assert ia.tobytes() == ib.tobytes(), "instance records"
    assert len(pa) == len(pb)
    if exact or pa.tobytes() == pb.tobytes():
        assert pa.tobytes() == pb.tobytes(), "pair records"
        return
    for f in ("lo0", "hi0", "cull0", "lo1", "hi1", "cull1"):
        assert pa[f].tobytes() == pb[f].tobytes(), f
    for f in ("ref0", "ref1"):
        ra, rb = pa[f].astype(np.int64), pb[f].astype(np.int64)
        tri_leaf = (ra < 0) & ((~ra & 15) != 0)
        assert np.array_equal(tri_leaf, (rb < 0) & ((~rb & 15) != 0)) and np.array_equal(ra[~tri_leaf], rb[~tri_leaf])
        assert np.array_equal(~ra[tri_leaf] & 15, ~rb[tri_leaf] & 15)


# ---- 1. the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [0, -1])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_records_equal_a_full_upload_of_the_refit_scene(built, name, max_leaf):
    base, moved, refit = cases.case(name)
    a, b = updated(base, moved, max_leaf_tris=max_leaf), make_hip_tracer(refit, W, H, max_leaf_tris=max_leaf)
    try:
        before = make_hip_tracer(base, W, H, max_leaf_tris=max_leaf)
        try:
            assert before.read_scene_records()[1].tobytes() != a.read_scene_records()[1].tobytes()
        finally:
            before.Close()
        same_records(a.read_scene_records(), b.read_scene_records(), exact=max_leaf == 0 or base.num_triangles > 2046)
    finally:
        a.Close()
        b.Close()


# ---- 2. results ----------------------------------------------------------------------------------------------------------------
def probe_rays(sc, n=20000, seed=3):
    rng = np.random.default_rng(seed)
    lo, hi = sc.bvh_nodes[0]["min"], sc.bvh_nodes[0]["max"]
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), size=(n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3] = np.where(rng.random(n) < 0.5, np.float32(3.402823466e+38), rng.uniform(0.05, 3.0, n)).astype(np.float32)
    return rays


VARIANTS = {
    "moving-0-8": [{}, {"traversal": 0}, {"node_mode": 0}, {"node_mode": 1}, {"node_mode": 2}],
    "transformed-returned": [{}, {"traversal": 0}, {"node_mode": 0}, {"node_mode": 1}],
    "one-instance": [{}, {"packet_primary": 1}, {"traversal": 0, "packet_primary": 0}, {"node_mode": 1}],
    "swarm-150": [{}, {"node_mode": 0}],
    "swarm-17-singular": [{}],
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_results_equal_a_full_upload_and_the_oracle(built, oracle, name):
    from oracle import pybind as ob

    base, moved, refit = cases.case(name)
    seeds = scenes.make_seeds(SPP, B, base=21)
    want, ws, wt = oracle.trace(refit, ob.make_request(W, H, spp=SPP, bounces=B), seeds, tap_sample=0)
    rays = probe_rays(refit)
    whit, wwuvt, wtri = oracle.intersect(refit, rays, any_hit=False)[:3]
    wocc = oracle.intersect(refit, rays, any_hit=True)[0]
    assert np.abs(want[..., :3]).sum() > 0 and 0 < (whit != 0).sum() < len(rays)
    for opts in VARIANTS[name]:
        a, b = updated(base, moved, **opts), make_hip_tracer(refit, W, H, **opts)
        try:
            for tr in (a, b):
                tr.set_option("time_kernels", 1)
            fa, fb = frame(a), frame(b)                         # batched, all counters
            assert np.array_equal(bits(fa[0]), bits(fb[0])) and fa[1] == fb[1], opts
            assert fa[1][:2] == (list(ws.rays_per_bounce[:B]), list(ws.occl_per_bounce[:B])), opts
            for k in ("intersect", "occlusion"):
                assert a.kernel_symbol(k) == b.kernel_symbol(k) != "", (k, opts)
            for tr in (a, b):
                tr.set_option("exact_accumulate", 1)
            ea, eb = frame(a), frame(b)
            assert np.array_equal(bits(ea[0]), bits(eb[0])) and ea[1] == eb[1], opts
            assert np.array_equal(bits(ea[0][..., :3]), bits(want[..., :3])), opts
            for any_hit in (False, True):
                ha, hb = a.probe_intersect(rays, any_hit=any_hit), b.probe_intersect(rays, any_hit=any_hit)
                assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(ha, hb)), (any_hit, opts)
                if any_hit:
                    assert np.array_equal(ha[0] != 0, np.asarray(wocc) != 0), opts
                else:
                    found = np.asarray(whit) != 0
                    assert np.array_equal(ha[0] != 0, found) and np.array_equal(ha[2][found], np.asarray(wtri)[found, 1]), opts
                    assert np.array_equal(bits(ha[1][found]), bits(np.asarray(wwuvt, np.float32)[found])), opts
            req = ob.make_request(W, H, spp=SPP, bounces=B)
            ta, tb = a.tap_primary(req, int(seeds[0])), b.tap_primary(req, int(seeds[0]))
            for k in ta:
                assert np.array_equal(bits(ta[k]), bits(tb[k])), (k, opts)
            for k in ("primary_hit", "primary_wuvt", "primary_tri"):
                assert np.array_equal(bits(ta[k]), bits(np.asarray(wt[k]).reshape(ta[k].shape))), (k, opts)
        finally:
            a.Close()
            b.Close()


# ---- 3. / 4. sequences -----------------------------------------------------------------------------------------------------------
def test_two_updates_equal_one_and_an_update_back_restores_the_upload(built):
    s0, s1, s2 = (scenes.moving_instances(k) for k in range(3))
    a, b = make_hip_tracer(s0, W, H, instance_update=1), make_hip_tracer(s0, W, H, instance_update=1)
    try:
        first = a.read_scene_records()
        f0 = frame(a)
        a.update_instances(*scenes.instance_update_args(scenes.refit_instances(s0, s1)))
        a.update_instances(*scenes.instance_update_args(scenes.refit_instances(s0, s2)))
        b.update_instances(*scenes.instance_update_args(scenes.refit_instances(s0, s2)))
        ra, rb = a.read_scene_records(), b.read_scene_records()
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()
        assert ra[1].tobytes() != first[1].tobytes()
        fa, fb = frame(a), frame(b)
        assert np.array_equal(bits(fa[0]), bits(fb[0])) and fa[1] == fb[1] and not np.array_equal(bits(fa[0]), bits(f0[0]))
        a.update_instances(*scenes.instance_update_args(s0))
        back = a.read_scene_records()
        assert back[0].tobytes() == first[0].tobytes() and back[1].tobytes() == first[1].tobytes()
        fr = frame(a)
        assert np.array_equal(bits(fr[0]), bits(f0[0])) and fr[1] == f0[1]
    finally:
        a.Close()
        b.Close()


# ---- 5. a light on a moved instance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["transformed-returned", "panel-light"])
def test_emissive_on_a_moved_instance_follows_and_a_null_list_leaves_it_behind(built, name):
    """transformed_instances' panel turns with its instance: the frame equals B's.  Whether a frame can SEE the emissive's transform
    is shown on panel-light: transformed_instances' light is sampled 3.5 below its ground (the reference takes the sample points
    through the inverse matrix, quirk a-9(4)), where every shadow ray is occluded -- the oracle's frame of that scene with the stale
    list is the same frame (0 of 3 072 pixels differ; panel-light: 1 611)."""
    base, moved, refit = cases.case(name)
    assert base.emissives.tobytes() != moved.emissives.tobytes()
    inv, boxes, ems = scenes.instance_update_args(moved)
    a, b, c = updated(base, moved), make_hip_tracer(refit, W, H), make_hip_tracer(base, W, H, instance_update=1)
    try:
        c.update_instances(inv, boxes, None)
        fa, fb, fc = frame(a), frame(b), frame(c)
        assert np.array_equal(bits(fa[0]), bits(fb[0])) and fa[1] == fb[1]
        if name == "panel-light":
            assert not np.array_equal(bits(fa[0]), bits(fc[0]))     # the test can see the light
        c.update_instances(inv, boxes, ems)
        fc = frame(c)
        assert np.array_equal(bits(fc[0]), bits(fa[0])) and fc[1] == fa[1]
    finally:
        for tr in (a, b, c):
            tr.Close()


# ---- 6. temporal history -------------------------------------------------------------------------------------------------------
def temporal_run(object_motion, use_update):
    s0, s1 = scenes.moving_instances(0), scenes.moving_instances(1)
    refit = scenes.refit_instances(s0, s1)
    tr = make_hip_tracer(s0, W, H, instance_update=1, object_motion=int(object_motion))
    try:
        tr.set_denoise(**T.DENOISE_DEFAULTS)
        tr.set_temporal(**T.TEMPORAL_DEFAULTS)
        trace(tr, W, H, 4, bounces=B)
        sync(tr, W, H, 4)
        if use_update:
            tr.update_instances(*scenes.instance_update_args(refit))
        else:
            upload(tr, refit)
        trace(tr, W, H, 1, base=9, bounces=B)
        sync(tr, W, H, 1)
        return {"prior": tr.read_aov(T.AOV_PRIOR), "temporal": tr.read_aov(T.AOV_TEMPORAL), "denoised": tr.read_aov(T.AOV_DENOISED),
                "framebuffer": tr.read_framebuffer()}
    finally:
        tr.Close()


@pytest.mark.parametrize("object_motion", [True, False])
def test_history_is_treated_as_by_an_upload(built, object_motion):
    got, want = temporal_run(object_motion, True), temporal_run(object_motion, False)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    m = got["prior"][..., 3]
    if object_motion:
        assert (m > 0).mean() > 0.5      # the history survived the move
    else:
        assert not (m > 0).any()         # dropped, as an upload drops it


# ---- 7. option off -------------------------------------------------------------------------------------------------------------
def test_option_off_changes_nothing_allocates_nothing_and_refuses(built):
    from polaris_amd.tracer import TracerError

    base, moved, _ = cases.case("moving-0-1")
    owned, frames, symbols = {}, {}, {}
    for how in ("never heard", "off", "on"):
        opts = {} if how == "never heard" else {"instance_update": int(how == "on")}
        tr = make_hip_tracer(base, W, H, **opts)
        try:
            owned[how] = tr.scene_counts()[2:]      # (allocations, bytes) the scene owns: free device memory is everybody's, this is exact
            tr.set_option("time_kernels", 1)
            frames[how] = frame(tr)
            symbols[how] = {k: tr.kernel_symbol(k) for k in ("generate", "intersect", "intersect_packet", "shade_first", "shade_sort", "shade_wave",
                                                             "scan", "occlusion", "fold", "resolve", "instance_extent", "repad", "refit_top")}
            if how != "on":
                with pytest.raises(TracerError) as e:
                    tr.update_instances(*scenes.instance_update_args(moved))
                assert e.value.code == E_UNSUPPORTED
                again = frame(tr)
                assert np.array_equal(bits(again[0]), bits(frames[how][0])) and again[1] == frames[how][1]
        finally:
            tr.Close()
    assert owned["off"] == owned["never heard"]
    assert owned["on"][0] == owned["off"][0] + 9 and owned["on"][1] > owned["off"][1]     # the plan's five arrays, four scratch arrays
    assert symbols["off"] == symbols["never heard"] and symbols["off"]["refit_top"] == ""
    for how in ("off", "on"):
        assert np.array_equal(bits(frames[how][0]), bits(frames["never heard"][0])) and frames[how][1] == frames["never heard"][1]


def test_reupload_replaces_everything(built):
    """Nothing of an uploaded scene outlives the next upload: tracer A uploads the cubes with instance_update, vertex_update and
    object_motion on and syncs a frame under temporal reuse, turns the three options off and uploads the one-instance Cornell box; it
    then owns, holds, traces, selects and refuses exactly what tracer B does, which only ever saw the Cornell box."""
    from oracle import pybind as ob
    from polaris_amd.tracer import ChangeType, HipTracer, TracerError, UpdateMode

    first, second = scenes.SCENES["cubes"](), cases.case("one-instance")[0]
    w = h = 32
    on = ("instance_update", "vertex_update", "object_motion")
    a, b = HipTracer("a", 0), make_hip_tracer(second, w, h)
    try:
        a.Init()
        for k in on:
            a.set_option(k, 1)
        a.set_temporal(**T.TEMPORAL_DEFAULTS)
        a.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (w, h))
        upload(a, first)
        a.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, first)
        trace(a, w, h, 1, bounces=2)
        sync(a, w, h, 1)
        assert a.scene_counts()[2] > b.scene_counts()[2]      # (A held both plans)
        for k in on:
            a.set_option(k, 0)
        upload(a, second)
        a.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, second)
        assert a.scene_counts() == b.scene_counts()            # pair records, instance records, allocations, bytes
        ra, rb = a.read_scene_records(), b.read_scene_records()
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()
        frames = []
        for tr in (a, b):
            tr.set_option("time_kernels", 1)
            tr.Trace(ob.make_request(w, h, spp=1, bounces=2), scenes.make_seeds(1, 2, base=21))
            frames.append((tr.read_accumulator(0), tr.last_trace_stats))
        assert np.array_equal(bits(frames[0][0]), bits(frames[1][0])) and np.abs(frames[0][0][..., :3]).sum() > 0
        assert list(frames[0][1].rays_per_bounce[:2]) == list(frames[1][1].rays_per_bounce[:2])
        assert a.kernel_symbol("intersect") == b.kernel_symbol("intersect") != ""
        codes = {}
        for name, tr in (("a", a), ("b", b)):
            for call, args in ((tr.update_instances, scenes.instance_update_args(second)), (tr.update_vertices, scenes.vertex_update_args(second))):
                with pytest.raises(TracerError) as e:
                    call(*args)
                codes.setdefault(name, []).append(e.value.code)
        assert codes["a"] == codes["b"] == [E_UNSUPPORTED, E_UNSUPPORTED]
    finally:
        a.Close()
        b.Close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_next_frame_as_the_one_before(built):
    from polaris_amd.tracer import ErrNoSceneData, HipTracer, TracerError
    from test_instance_update_cpu import _refusals

    base, moved, _ = cases.case("transformed-returned")
    tr = make_hip_tracer(base, W, H, instance_update=1)
    try:
        f0, r0 = frame(tr), tr.read_scene_records()
        for what, status, (u, keep), option_on in _refusals(base, moved):
            if not option_on:
                continue                                        # (test_option_off_...)
            rc = tr._lib.polaris_hip_update_instances(tr._h, C.byref(u))
            assert rc == status, (what, rc)
            assert tr._lib.polaris_hip_last_error(tr._h)
            r = tr.read_scene_records()
            assert r[0].tobytes() == r0[0].tobytes() and r[1].tobytes() == r0[1].tobytes(), what
            f = frame(tr)
            assert np.array_equal(bits(f[0]), bits(f0[0])) and f[1] == f0[1], what
        assert tr._lib.polaris_hip_update_instances(tr._h, None) == E_BAD_ARGUMENT
    finally:
        tr.Close()
    early = HipTracer("early", 0)
    early.Init()
    try:
        with pytest.raises(ErrNoSceneData):
            early.update_instances(*scenes.instance_update_args(moved))
    finally:
        early.Close()


# ---- 9. far moves --------------------------------------------------------------------------------------------------------------
def test_a_move_far_outside_the_room_is_repadded_not_refused(built):
    """The boxes leaf subdivision added are padded by 2^-13 of the scene's extent in the mesh's space, which a far move multiplies.
    The update gives them the padding a full upload would (k_repad), so it needs no refusal: records and frame equal B's."""
    base = scenes.moving_instances(0)
    inv, boxes, ems = scenes.instance_update_args(base)
    far = scenes.translation((40.0, 0.0, 25.0))
    fwd = far @ np.linalg.inv(inv[2].reshape(4, 4).T.astype(np.float64))
    inv[2] = np.linalg.inv(fwd).T.reshape(-1).astype(np.float32)
    boxes[2, :3] += np.float32([40.0, 0.0, 25.0])
    boxes[2, 3:] += np.float32([40.0, 0.0, 25.0])
    moved = scenes.refit_instances(base, base)
    moved.mesh_instances["inv_transform"] = inv
    idx, _ = scenes._top_level_nodes(moved)
    leaf = idx[moved.bvh_nodes["ldata"][idx] <= 0]
    which = -moved.bvh_nodes["ldata"][leaf].astype(np.int64)
    moved.bvh_nodes["min"][leaf], moved.bvh_nodes["max"][leaf] = boxes[which, :3], boxes[which, 3:]
    refit = scenes.refit_instances(base, moved)
    a, b = updated(base, refit), make_hip_tracer(refit, W, H)
    try:
        ra, first = a.read_scene_records(), make_hip_tracer(base, W, H)
        try:
            changed = np.array([x.tobytes() != y.tobytes() for x, y in zip(first.read_scene_records()[0], ra[0])])
        finally:
            first.Close()
        assert changed.sum() > 2                                # mesh-level boxes were re-padded, not only the two top-level records
        same_records(ra, b.read_scene_records(), exact=base.num_triangles > 2046)
        fa, fb = frame(a), frame(b)
        assert np.array_equal(bits(fa[0]), bits(fb[0])) and fa[1] == fb[1]
    finally:
        a.Close()
        b.Close()


# ---- 10. the host layer --------------------------------------------------------------------------------------------------------
def test_renderer_forwards_the_update_to_every_tracer(built):
    """Renderer.update_instances (polaris_host_renderer_update_instances) on two tracers sharing the frame: the frame equals that of a
    renderer that uploaded the refit scene; before its scene was uploaded with the option on, the renderer refuses."""
    from polaris_amd import host_api

    host_api.load()
    base, moved, refit = cases.case("moving-0-8")
    spp = 2

    def render(r):
        for t in range(2):
            r.push_seeds(t, scenes.make_seeds(spp, B, base=31 + t))
        r.render()
        return r.read()

    a = host_api.Renderer(base, [0, 0], width=W, height=H, spp=spp, bounces=B, seed=4)
    b = host_api.Renderer(refit, [0, 0], width=W, height=H, spp=spp, bounces=B, seed=4)
    try:
        with pytest.raises(RuntimeError, match="instance_update off"):
            a.update_instances(*scenes.instance_update_args(moved))
        a.set_option("instance_update", 1)
        a.upload_scene(base)
        f0 = render(a)
        a.update_instances(*scenes.instance_update_args(moved))
        fa, fb = render(a), render(b)
        assert np.array_equal(bits(fa[1]), bits(fb[1])) and np.array_equal(fa[0], fb[0])
        assert not np.array_equal(bits(fa[1]), bits(f0[1]))
    finally:
        a.close()
        b.close()
