"""Deforming meshes in place on the MI355X (polaris_hip_update_vertices, option "vertex_update").

Set-up: tracer A uploads `base` with the option on and calls update_vertices with `refit`'s vertices, boxes and emissives (normals and
matrices where the case passes them); tracer B uploads `refit` = scenes.refit_vertices(base, ...), the scene the update is defined to
equal; the CPU oracle traces refit's arrays.  Bars: at max_leaf_tris = 0 the device's pair and instance records of A and B are
byte-equal (a scene of at most 2 046 slots: up to the slot a triangle-leaf reference names, tests/test_vertex_update_cpu.py resolves
those); frames, counters, probes and taps of A, of B and of the oracle are bit-equal whatever traversal kernel runs; the temporal
history is dropped; with the option off nothing changes, nothing is allocated, and the call is refused; a refused call leaves the next
frame bit-equal to the frame before it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import vertex_update_cases as cases
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from polaris_amd import scenes
from test_gpu_denoise import sync, trace
from test_gpu_instance_update import B, H, SPP, W, counters, frame, probe_rays, same_records

pytestmark = pytest.mark.gpu

E_BAD_ARGUMENT, E_BAD_SCENE, E_UNSUPPORTED = 2, 5, 6
NOT_TINY = ("grid-64", "big-leaves")


def updated(name, **options):
    base, _, _ = cases.case(name)
    tr = make_hip_tracer(base, W, H, vertex_update=1, **options)
    tr.update_vertices(*cases.update_args(name))
    return tr


def same_frame(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1]


# ---- 1. the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_records_equal_a_full_upload_of_the_refit_scene(built, name):
    base, refit, _ = cases.case(name)
    a, b, before = updated(name, max_leaf_tris=0), make_hip_tracer(refit, W, H, max_leaf_tris=0), make_hip_tracer(base, W, H, max_leaf_tris=0)
    try:
        ra, rb, r0 = a.read_scene_records(), b.read_scene_records(), before.read_scene_records()
        assert ra[0].tobytes() != r0[0].tobytes()
        same_records(ra, rb, exact=name in NOT_TINY)
    finally:
        for tr in (a, b, before):
            tr.Close()


# ---- 2. results ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_results(name):
    """What the CPU oracle makes of the refit scene, once per case."""
    from oracle import pybind as ob

    _, refit, _ = cases.case(name)
    oracle = ob.Oracle("oracle")
    seeds = scenes.make_seeds(SPP, B, base=21)
    want, ws, wt = oracle.trace(refit, ob.make_request(W, H, spp=SPP, bounces=B), seeds, tap_sample=0)
    rays = probe_rays(refit)
    whit, wwuvt, wtri = oracle.intersect(refit, rays, any_hit=False)[:3]
    wocc = oracle.intersect(refit, rays, any_hit=True)[0]
    assert np.abs(want[..., :3]).sum() > 0 and 0 < (np.asarray(whit) != 0).sum() < len(rays)
    return seeds, want, ws, wt, rays, np.asarray(whit), np.asarray(wwuvt, np.float32), np.asarray(wtri), np.asarray(wocc)


def variants(name):
    out = [{}, {"traversal": 0}, {"node_mode": 0}, {"node_mode": 1}, {"packet_primary": 1}]
    return out if name in NOT_TINY else out + [{"node_mode": 2}]


@pytest.mark.parametrize("max_leaf", [-1, 0])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_results_equal_a_full_upload_and_the_oracle(built, oracle, name, max_leaf):
    from oracle import pybind as ob

    _, refit, _ = cases.case(name)
    seeds, want, ws, wt, rays, whit, wwuvt, wtri, wocc = oracle_results(name)
    for opts in variants(name):
        opts = dict(opts, max_leaf_tris=max_leaf)
        a, b = updated(name, **opts), make_hip_tracer(refit, W, H, **opts)
        try:
            for tr in (a, b):
                tr.set_option("time_kernels", 1)
            fa, fb = frame(a), frame(b)                         # batched, all counters
            assert same_frame(fa, fb), opts
            assert fa[1][:2] == (list(ws.rays_per_bounce[:B]), list(ws.occl_per_bounce[:B])), opts
            for k in ("intersect", "occlusion"):
                assert a.kernel_symbol(k) == b.kernel_symbol(k) != "", (k, opts)
            for tr in (a, b):
                tr.set_option("exact_accumulate", 1)
            ea, eb = frame(a), frame(b)
            assert same_frame(ea, eb), opts
            assert np.array_equal(bits(ea[0][..., :3]), bits(want[..., :3])), opts
            for any_hit in (False, True):
                ha, hb = a.probe_intersect(rays, any_hit=any_hit), b.probe_intersect(rays, any_hit=any_hit)
                assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(ha, hb)), (any_hit, opts)
                if any_hit:
                    assert np.array_equal(ha[0] != 0, wocc != 0), opts
                else:
                    found = whit != 0
                    assert np.array_equal(ha[0] != 0, found) and np.array_equal(ha[2][found], wtri[found, 1]), opts
                    assert np.array_equal(bits(ha[1][found]), bits(wwuvt[found])), opts
            req = ob.make_request(W, H, spp=SPP, bounces=B)
            ta, tb = a.tap_primary(req, int(seeds[0])), b.tap_primary(req, int(seeds[0]))
            for k in ta:
                assert np.array_equal(bits(ta[k]), bits(tb[k])), (k, opts)
            for k in ("primary_hit", "primary_wuvt", "primary_tri"):
                assert np.array_equal(bits(ta[k]), bits(np.asarray(wt[k]).reshape(ta[k].shape))), (k, opts)
        finally:
            a.Close()
            b.Close()


# ---- 3. sequences --------------------------------------------------------------------------------------------------------------
def test_two_updates_equal_one_and_an_update_back_restores_the_upload(built):
    name = "cubes-shared-mesh"
    base, refit, _ = cases.case(name)
    other = scenes.refit_vertices(base, cases.deformed(base, 33, 0.15, cases.mesh_vertex_mask(base, 1)))
    a, b = make_hip_tracer(base, W, H, vertex_update=1, max_leaf_tris=0), make_hip_tracer(base, W, H, vertex_update=1, max_leaf_tris=0)
    try:
        first, f0 = a.read_scene_records(), frame(a)
        a.update_vertices(*scenes.vertex_update_args(other))
        a.update_vertices(*cases.update_args(name))
        b.update_vertices(*cases.update_args(name))
        ra, rb = a.read_scene_records(), b.read_scene_records()
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[0].tobytes() != first[0].tobytes()
        fa, fb = frame(a), frame(b)
        assert same_frame(fa, fb) and not np.array_equal(bits(fa[0]), bits(f0[0]))
        # back to the base's own vertices and boxes: the base's mesh boxes are the scene builder's minima / maxima, the update's are
        # the fold's -- the same bytes wherever no +0 meets a -0 (the base's zeros are all +0)
        a.update_vertices(*scenes.vertex_update_args(base))
        back = a.read_scene_records()
        assert back[0].tobytes() == first[0].tobytes() and back[1].tobytes() == first[1].tobytes()
        assert same_frame(frame(a), f0)
    finally:
        a.Close()
        b.Close()


@pytest.mark.parametrize("vertices_first", [True, False])
def test_vertex_and_instance_updates_compose_in_either_order(built, vertices_first):
    """update_vertices then update_instances, and the reverse, equal a fresh upload of the scene that is both deformed and moved: the
    instance update sees the deformed meshes' boxes and bounds, the vertex update the current matrices."""
    name = "moving-and-deformed"
    base, both, _ = cases.case(name)
    moved = scenes.refit_instances(base, scenes.moving_instances(1))
    only_deformed = scenes.refit_vertices(base, both.vertices)
    a, b = make_hip_tracer(base, W, H, vertex_update=1), make_hip_tracer(both, W, H)
    try:
        if vertices_first:
            vertices, boxes, _, _, ems = scenes.vertex_update_args(only_deformed)
            a.update_vertices(vertices, boxes, None, None, ems)
            a.update_instances(*scenes.instance_update_args(both))
        else:
            a.update_instances(*scenes.instance_update_args(moved))
            vertices, boxes, _, _, ems = scenes.vertex_update_args(both)
            a.update_vertices(vertices, boxes, None, None, ems)       # (matrices NULL: the ones update_instances set stay)
        same_records(a.read_scene_records(), b.read_scene_records(), exact=False)
        assert same_frame(frame(a), frame(b))
        for tr in (a, b):
            tr.set_option("exact_accumulate", 1)
        assert same_frame(frame(a), frame(b))
    finally:
        a.Close()
        b.Close()


# ---- 4. / 5. light and normals -------------------------------------------------------------------------------------------------
def test_stretched_light_panel_follows(built, oracle):
    from oracle import pybind as ob

    base, refit, _ = cases.case("panel-light")
    assert (base.emissives["area"] != refit.emissives["area"]).any()
    a, c = updated("panel-light"), make_hip_tracer(base, W, H)
    try:
        for tr in (a, c):
            tr.set_option("exact_accumulate", 1)
        fa, fc = frame(a), frame(c)
        want = oracle.trace(refit, ob.make_request(W, H, spp=SPP, bounces=B), scenes.make_seeds(SPP, B, base=21))[0]
        assert np.array_equal(bits(fa[0][..., :3]), bits(want[..., :3]))
        assert not np.array_equal(bits(fa[0]), bits(fc[0]))
    finally:
        a.Close()
        c.Close()


def test_new_normals_show_and_null_normals_stay(built):
    frames = {}
    for name in ("sphere-normals", "sphere-null-normals"):
        _, refit, _ = cases.case(name)
        a, b = updated(name), make_hip_tracer(refit, W, H)
        try:
            frames[name] = frame(a)
            assert same_frame(frames[name], frame(b)), name
        finally:
            a.Close()
            b.Close()
    assert not np.array_equal(bits(frames["sphere-normals"][0]), bits(frames["sphere-null-normals"][0]))


# ---- 6. G-buffer and history ---------------------------------------------------------------------------------------------------
def test_gbuffer_after_the_update_equals_a_full_upload(built):
    name = "cornell"
    _, refit, _ = cases.case(name)
    a, b = make_hip_tracer(cases.case(name)[0], W, H, vertex_update=1), make_hip_tracer(refit, W, H)
    try:
        stale = a.read_aov(T.AOV_GUIDE)                        # the G-buffer of the base scene: the update must invalidate it
        a.update_vertices(*cases.update_args(name))
        for aov in (T.AOV_GUIDE, T.AOV_ALBEDO):
            assert np.array_equal(bits(a.read_aov(aov)), bits(b.read_aov(aov))), aov
        assert not np.array_equal(bits(a.read_aov(T.AOV_GUIDE)), bits(stale))
    finally:
        a.Close()
        b.Close()


@pytest.mark.parametrize("object_motion", [True, False])
def test_history_is_dropped(built, object_motion):
    name = "moving-and-deformed"
    base, refit, _ = cases.case(name)

    def run(tr, with_update):
        try:
            tr.set_denoise(**T.DENOISE_DEFAULTS)
            tr.set_temporal(**T.TEMPORAL_DEFAULTS)
            if with_update:
                trace(tr, W, H, 4, bounces=B)
                sync(tr, W, H, 4)
                tr.update_vertices(*cases.update_args(name))
            trace(tr, W, H, 1, base=9, bounces=B)
            sync(tr, W, H, 1)
            return tr.read_aov(T.AOV_PRIOR), tr.read_framebuffer()
        finally:
            tr.Close()

    prior, fb = run(make_hip_tracer(base, W, H, vertex_update=1, object_motion=int(object_motion)), True)
    _, want = run(make_hip_tracer(refit, W, H, object_motion=int(object_motion)), False)
    assert not (prior[..., 3] != 0).any()                       # no history: m = 0 everywhere
    assert np.array_equal(fb, want)


# ---- 7. option off -------------------------------------------------------------------------------------------------------------
def test_option_off_changes_nothing_allocates_nothing_and_refuses(built):
    from polaris_amd.tracer import TracerError

    name = "moving-and-deformed"
    base, _, _ = cases.case(name)
    timers = ("generate", "intersect", "intersect_packet", "shade_first", "shade_sort", "shade_wave", "scan", "occlusion", "fold", "resolve",
              "instance_extent", "repad", "refit_top", "tri_records", "refit_mesh")
    owned, frames, symbols = {}, {}, {}
    for how in ("never heard", "off", "instance", "on"):
        opts = {"never heard": {}, "off": {"vertex_update": 0}, "instance": {"instance_update": 1}, "on": {"vertex_update": 1}}[how]
        tr = make_hip_tracer(base, W, H, **opts)
        try:
            owned[how] = tr.scene_counts()[2:]      # (allocations, bytes) the scene owns
            tr.set_option("time_kernels", 1)
            frames[how] = frame(tr)
            symbols[how] = {k: tr.kernel_symbol(k) for k in timers}
            if how != "on":
                with pytest.raises(TracerError) as e:
                    tr.update_vertices(*cases.update_args(name))
                assert e.value.code == E_UNSUPPORTED
                assert same_frame(frame(tr), frames[how])
            else:
                tr.update_instances(*scenes.instance_update_args(base))      # the option keeps what the instance update needs too
                tr.update_vertices(*cases.update_args(name))
                assert tr.kernel_symbol("tri_records") == "pol::k_tri_records" and tr.kernel_symbol("refit_mesh") == "pol::k_refit_mesh"
                assert all(tr.kernel_ms(k)[1] > 0 for k in ("tri_records", "refit_mesh", "instance_extent", "refit_top"))
        finally:
            tr.Close()
    assert owned["off"] == owned["never heard"]
    assert owned["on"][0] == owned["instance"][0] + 5 and owned["on"][1] > owned["instance"][1]     # the mesh plan's three arrays, two scratch arrays
    assert symbols["off"] == symbols["never heard"] and symbols["off"]["refit_mesh"] == "" and symbols["off"]["tri_records"] == ""
    for how in ("off", "instance", "on"):
        assert same_frame(frames[how], frames["never heard"]), how


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_next_frame_as_the_one_before(built):
    from polaris_amd.tracer import ErrNoSceneData, HipTracer
    from test_vertex_update_cpu import _refusals, shared_subtree_scene

    name = "moving-and-deformed"
    base, _, _ = cases.case(name)
    tr = make_hip_tracer(base, W, H, vertex_update=1)
    try:
        f0, r0 = frame(tr), tr.read_scene_records()
        for what, status, text, (u, keep), option_on in _refusals(name):
            if not option_on:
                continue                                        # (test_option_off_...)
            rc = tr._lib.polaris_hip_update_vertices(tr._h, C.byref(u))
            assert rc == status, (what, rc)
            assert text.encode() in tr._lib.polaris_hip_last_error(tr._h), what
            r = tr.read_scene_records()
            assert r[0].tobytes() == r0[0].tobytes() and r[1].tobytes() == r0[1].tobytes(), what
            assert same_frame(frame(tr), f0), what
        assert tr._lib.polaris_hip_update_vertices(tr._h, None) == E_BAD_ARGUMENT
    finally:
        tr.Close()
    shared, _ = shared_subtree_scene()
    tr = make_hip_tracer(shared, W, H, vertex_update=1)         # uploads fine ...
    try:
        f0 = frame(tr)
        u, keep = T.vertex_update(*scenes.vertex_update_args(shared))
        assert tr._lib.polaris_hip_update_vertices(tr._h, C.byref(u)) == E_UNSUPPORTED      # ... and is refused by name
        assert b"shared by two mesh trees" in tr._lib.polaris_hip_last_error(tr._h)
        tr.update_instances(*scenes.instance_update_args(shared))           # (the instance plan was kept)
        assert same_frame(frame(tr), f0)
    finally:
        tr.Close()
    early = HipTracer("early", 0)
    early.Init()
    try:
        with pytest.raises(ErrNoSceneData):
            early.update_vertices(*cases.update_args(name))
    finally:
        early.Close()


# ---- 9. the host layer ---------------------------------------------------------------------------------------------------------
def test_renderer_forwards_the_update_to_every_tracer(built):
    from polaris_amd import host_api

    host_api.load()
    name = "moving-and-deformed"
    base, refit, _ = cases.case(name)
    spp = 2

    def render(r):
        for t in range(2):
            r.push_seeds(t, scenes.make_seeds(spp, B, base=31 + t))
        r.render()
        return r.read()

    a = host_api.Renderer(base, [0, 0], width=W, height=H, spp=spp, bounces=B, seed=4)
    b = host_api.Renderer(refit, [0, 0], width=W, height=H, spp=spp, bounces=B, seed=4)
    try:
        with pytest.raises(RuntimeError, match="vertex_update off"):
            a.update_vertices(*cases.update_args(name))
        a.set_option("vertex_update", 1)
        a.upload_scene(base)
        f0 = render(a)
        a.update_vertices(*cases.update_args(name))
        fa, fb = render(a), render(b)
        assert np.array_equal(bits(fa[1]), bits(fb[1])) and np.array_equal(fa[0], fb[0])
        assert not np.array_equal(bits(fa[1]), bits(f0[1]))
    finally:
        a.close()
        b.close()
