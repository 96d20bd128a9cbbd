"""The orthographic and equirectangular cameras on the MI355X (include/polaris_hip.h: polaris_hip_set_projection).

Bars: with kind = 0 (and garbage in the other fields) a tracer is bit for bit the tracer that never heard of the projection, under the
same kernel symbols; with it on, polaris_hip_tap_primary's rays are tests/projection_oracle.py's bit for bit and their hits the
oracle's on those rays; GUIDE t and the hit pattern are the oracle's on the restated centre rays; the image does not depend on which
traversal / shade kernel family ran nor on the batch size; on -> off -> on returns to the first frame through the perspective
tracer's; every refusal leaves the next frame as it was; after a translation of the eye PRIOR is the host restatement's on the
device's own planes, after a set_camera with the same eye every filtered pixel takes history, a changed projection drops the history
and the G-buffer and an equal one keeps both; HipTracer.set_projection is set_projection_params with the derived basis.

Frames: 16 x 9 (N = 144: one partly filled chunk) and 40 x 20 (N = 800: three full chunks and a tail).  3 spp, 3 bounces.  The basis
is the frustum's, turned a few degrees about each of its vectors: no entry is 0 or -0.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gbuffer_oracle as GO
import projection_oracle as PO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_batched_exact import counters
from test_gpu_denoise import sync, trace
from test_gpu_parity import _nested_shells_scene

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES = [(16, 9), (40, 20)]
SPP, B, RR = 3, 3, 1
KINDS = [PO.ORTHOGRAPHIC, PO.EQUIRECTANGULAR]
PARTIAL = dict(lon_range=2 * np.pi / 3, lat_range=np.pi / 3)      # a third of the panorama each way: the scene fills the frame
SYMBOL = {PO.ORTHOGRAPHIC: "pol::k_generate_proj<1>", PO.EQUIRECTANGULAR: "pol::k_generate_proj<2>"}


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def request(W, H, spp=SPP, bounces=B, rr=RR):
    from oracle import pybind as ob

    return ob.make_request(W, H, spp=spp, bounces=bounces, rr=rr)


def seeds_of(spp=SPP, bounces=B, base=41):
    from polaris_amd import scenes

    return scenes.make_seeds(spp, bounces, base=base)


def cornell(W, H):
    from polaris_amd import scenes

    return scenes.SCENES["cornell"](W / H)


def image_projection(sc, kind):
    return PO.scene_projection(sc, kind, True, **(PARTIAL if kind == PO.EQUIRECTANGULAR else {}))


def set_cam(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)


def frame_of(tr, req, seeds):
    """One Trace into a cleared frame, merged and synced: (trace accumulator, counters, frame-buffer bytes)."""
    req.accumulated_samples = 0
    tr.Trace(req, seeds)
    acc, st = tr.read_accumulator(0), counters(tr.last_trace_stats, req.num_bounces)
    tr.MergeOutput(tr, req)
    tr.SyncFramebuffer(req)
    return acc, st, tr.read_framebuffer()


# ---- 1. off is off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
def test_kind_0_with_garbage_is_the_tracer_that_never_heard_of_it(built, frame):
    W, H = frame
    sc, seeds = cornell(W, H), seeds_of()
    moved = dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([0.02, 0.01, 0], F)).astype(F))
    garbage = T.projection_params(0, (np.nan, 1e30, -0.0), (np.inf, 2, 3), (0, 0, 0), -1.0, np.nan, 99.0, -np.inf)
    got = []
    for off_call in (False, True):
        tr = make_hip_tracer(sc, W, H, time_kernels=1)
        try:
            if off_call:
                tr.set_projection_params(garbage)
                tr.set_projection(None)
            tr.set_temporal()
            first = frame_of(tr, request(W, H), seeds)
            symbols = [tr.kernel_symbol("generate"), tr.kernel_symbol("gbuffer")]
            planes = [tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)]
            set_cam(tr, moved)
            second = frame_of(tr, request(W, H), seeds)
            symbols.append(tr.kernel_symbol("reproject"))
            planes += [tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_TEMPORAL)]
            got.append((first, second, symbols, planes))
        finally:
            tr.Close()
    a, b = got
    assert a[2] == b[2] == ["pol::k_generate", "pol::k_gbuffer", "pol::k_reproject<false, false>"]
    for x, y in ((a[0], b[0]), (a[1], b[1])):
        assert x[1] == y[1] and x[1][2] == W * H * SPP
        assert np.array_equal(bits(x[0]), bits(y[0])) and x[0][..., :3].any() and np.array_equal(x[2], y[2])
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(bits(x), bits(y))
    assert (a[3][2][..., 3] > 0).any()


# ---- 2. ray bits ----------------------------------------------------------------------------------------------------------------
def ray_scenes(W, H):
    from polaris_amd import scenes

    return {"cornell": (cornell(W, H), {}),                                                       # tiny-scene mode
            "moving-instances": (scenes.moving_instances(0, W / H), {}),
            "nested-shells": (_nested_shells_scene(), {"node_mode": 0, "max_leaf_tris": 0})}      # the tree stays in HBM, 24-entry stack


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["cornell", "moving-instances", "nested-shells"])
def test_tapped_rays_are_the_restatements_and_their_hits_the_oracles(built, oracle, name, frame):
    W, H = frame
    sc, options = ray_scenes(W, H)[name]
    tap_seeds = [7, 0x9E3779B9, 0xFFFFFFF0, 123456789]       # (0xFFFFFFF0: gx + seed wraps)
    cameras = [PO.scene_projection(sc, PO.ORTHOGRAPHIC), PO.scene_projection(sc, PO.EQUIRECTANGULAR), image_projection(sc, PO.EQUIRECTANGULAR)]
    want = {}
    for k, proj in enumerate(cameras):
        for seed in tap_seeds:
            rays = PO.projection_rays(oracle, sc.eye, proj, W, H, 0, H, seed)
            want[k, seed] = (rays,) + tuple(oracle.intersect(sc, rays))
        assert any(want[k, s][1].any() for s in tap_seeds), ("no restated ray hits the scene", k)
    for packet in (0, 1):
        tr = make_hip_tracer(sc, W, H, packet_primary=packet, **options)
        try:
            for k, proj in enumerate(cameras):
                tr.set_projection_params(proj.params())
                for seed in tap_seeds:
                    taps = tr.tap_primary(request(W, H), seed)
                    rays, hit, wuvt, it = want[k, seed]
                    what = (name, frame, packet, k, seed)
                    assert np.array_equal(bits(taps["primary_rays"]), bits(rays)), (what, int((bits(taps["primary_rays"]) != bits(rays)).sum()))
                    assert np.array_equal(taps["primary_hit"] != 0, hit != 0), what
                    h = hit != 0
                    assert np.array_equal(bits(taps["primary_wuvt"][h]), bits(wuvt[h])), what
                    assert np.array_equal(taps["primary_tri"][h], it[h]), what
        finally:
            tr.Close()


# ---- 3. the G-buffer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_guide_t_and_the_hit_pattern_are_the_oracles_on_the_restated_centre_rays(built, oracle, kind, frame):
    W, H = frame
    sc = cornell(W, H)
    proj = image_projection(sc, kind)
    rays = PO.centre_rays(oracle, sc.eye, proj, W, H)
    want_g, want_a = PO.gbuffer(oracle, sc, rays, W, H)
    hit = want_g[..., 3] < PO.FLT_MAX
    assert hit.sum() >= W * H // 8
    planes = {}
    for links in (0, 2):
        tr = make_hip_tracer(sc, W, H, guide_specular=links, time_kernels=1)
        try:
            tr.set_projection_params(proj.params())
            planes[links] = (tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO))
            assert tr.kernel_symbol("gbuffer") == ("pol::k_gbuffer_chain_proj" if links else "pol::k_gbuffer_proj")
        finally:
            tr.Close()
    guide, albedo = planes[0]
    assert np.array_equal(guide[..., 3] < PO.FLT_MAX, hit)
    assert np.array_equal(bits(guide[..., 3]), bits(want_g[..., 3]))
    assert np.array_equal(bits(albedo[..., 3]), bits(want_a[..., 3]))
    assert np.array_equal(bits(guide), bits(want_g)) and np.array_equal(bits(albedo), bits(want_a))
    # guide_specular = 2: wherever the first hit is no mirror and no glass the chain follows nothing and the planes are the first hit's
    leaf = bits(albedo[..., 3]).view(np.int32)
    first_hit = (leaf != T.BXDF_CONDUCTOR) & (leaf != T.BXDF_DIELECTRIC)
    assert (first_hit & hit).sum() >= W * H // 8
    assert np.array_equal(bits(planes[2][0][first_hit]), bits(guide[first_hit])) and np.array_equal(bits(planes[2][1][first_hit]), bits(albedo[first_hit]))


@pytest.mark.parametrize("frame", FRAMES)
def test_an_orthographic_camera_sees_the_back_wall_at_one_distance(built, frame):
    """Geometry, not rounding: looking along the box's depth axis every pixel whose first hit is the back wall has the same GUIDE t, the
    wall's distance from the eye's plane.  A wrong basis or window is off by percent."""
    W, H = frame
    sc = cornell(W, H)
    axis, right, up, _ = T.projection_from_frustum(sc.frustum)
    half = 0.45 * PO.scene_extent(sc)                                            # a square window inside the box's opening
    proj = PO.Projection(PO.ORTHOGRAPHIC, axis, right, up, half_width=half, half_height=half)
    k = int(np.argmax(np.abs(proj.axis)))
    assert abs(float(proj.axis[k])) > 0.9999 and float(proj.axis[k]) > 0        # the Cornell camera looks along a world axis
    wall = float(sc.bvh_nodes["max"].max(axis=0)[k])
    depth = wall - float(np.asarray(sc.eye, np.float64)[k])
    tr = make_hip_tracer(sc, W, H)
    try:
        tr.set_projection_params(proj.params())
        guide = tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    t, n = guide[..., 3].astype(np.float64), guide[..., :3].astype(np.float64)
    on_wall = (t < 1e30) & (np.abs(t - depth) <= 1e-3 * depth) & (n[..., k] < -0.99)      # the first hit lies in the wall's plane, facing the camera
    assert on_wall.sum() >= W * H // 8
    assert np.abs(t[on_wall] / depth - 1).max() <= 1e-4
    assert t[on_wall].max() / t[on_wall].min() - 1 <= 1e-4
    assert not (t[t < 1e30] > depth * (1 + 1e-4)).any()                                   # nothing is seen behind the back wall


# ---- 4. one image whichever kernel ----------------------------------------------------------------------------------------------
def projected_frame(sc, W, H, proj, seeds, spp=SPP, **options):
    moments = options.pop("moments", 0)
    tr = make_hip_tracer(sc, W, H, **options)
    try:
        if moments:
            tr.set_option("moments", 1)
        tr.set_projection_params(proj.params())
        tr.Trace(request(W, H, spp=spp), seeds)
        return tr.read_accumulator(0), counters(tr.last_trace_stats, B)
    finally:
        tr.Close()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_image_whichever_kernel_traces_and_shades_it(built, kind, frame):
    """traversal x packet_primary x the node modes the Cornell box admits, with o12 and shade_wave going through their combinations along
    the way, in exact and batched mode; then the batch sizes and the moments."""
    W, H = frame
    sc, seeds = cornell(W, H), seeds_of()
    proj = image_projection(sc, kind)
    grid = [dict(traversal=t, packet_primary=p, node_mode=n) for t in (1, 0) for p in (0, 1) for n in (2, 1, 0)]
    for exact in (1, 0):
        first = None
        for k, options in enumerate(grid):
            options = dict(options, o12=k & 1, shade_wave=(k >> 1) & 1, exact_accumulate=exact)
            acc, st = projected_frame(sc, W, H, proj, seeds, **options)
            if first is None:
                first = (acc, st)
                assert acc[..., :3].any() and st[2] == W * H * SPP and st[4] > 0
            assert st == first[1], (exact, options)
            assert np.array_equal(bits(acc), bits(first[0])), (exact, options, int((bits(acc) != bits(first[0])).sum()))
    ref, st = projected_frame(sc, W, H, proj, seeds, samples_per_batch=1, overlap=3)
    assert not bits(ref[..., 3]).any()
    for options in (dict(samples_per_batch=2, overlap=2), dict(samples_per_batch=3), dict(samples_per_batch=2, overlap=2, moments=1), dict(moments=1)):
        acc, st2 = projected_frame(sc, W, H, proj, seeds, **options)
        assert st2 == st, options
        assert np.array_equal(bits(acc[..., :3]), bits(ref[..., :3])), options
        assert bool(acc[..., 3].any()) == bool(options.get("moments")), options


# ---- 5. switching ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_on_off_on_returns_to_the_first_frame_through_the_perspective_tracers(built, kind, frame):
    W, H = frame
    sc, seeds = cornell(W, H), seeds_of()
    proj = image_projection(sc, kind)
    pin = make_hip_tracer(sc, W, H, time_kernels=1)
    tr = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        perspective = frame_of(pin, request(W, H), seeds)
        tr.set_projection_params(proj.params())
        first = frame_of(tr, request(W, H), seeds)
        assert tr.kernel_symbol("generate") == SYMBOL[kind]
        tr.set_projection(None)
        middle = frame_of(tr, request(W, H), seeds)
        assert tr.kernel_symbol("generate") == "pol::k_generate"
        tr.set_projection_params(proj.params())
        third = frame_of(tr, request(W, H), seeds)
    finally:
        pin.Close()
        tr.Close()
    for a, b, what in ((first, third, "first / third"), (middle, perspective, "middle / perspective")):
        assert a[1] == b[1], what
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2]), what
    assert not np.array_equal(bits(first[0]), bits(perspective[0]))      # (the projection does something)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def refused_params(good: T.ProjectionParams):
    def but(**kw):
        p = T.ProjectionParams()
        C.memmove(C.byref(p), C.byref(good), C.sizeof(p))
        for k, v in kw.items():
            if "_at_" in k:
                name, i = k.split("_at_")
                getattr(p, name)[int(i)] = v
            else:
                setattr(p, k, v)
        return p

    cases = [("struct_size 56", but(struct_size=56)), ("struct_size 64", but(struct_size=64)), ("kind 3", but(kind=3))]
    for field in ("axis_at_0", "right_at_1", "up_at_2", "half_width", "half_height", "lon_range", "lat_range"):
        for bad in (float("nan"), float("inf")):
            cases.append((f"{field} = {bad}", but(**{field: bad})))
    cases += [("zero axis", but(axis_at_0=0.0, axis_at_1=0.0, axis_at_2=0.0)), ("long up", but(up_at_0=good.up[0] * 1.01, up_at_1=good.up[1] * 1.01, up_at_2=good.up[2] * 1.01)),
              ("right is the axis", but(right_at_0=good.axis[0], right_at_1=good.axis[1], right_at_2=good.axis[2]))]
    if good.kind == PO.ORTHOGRAPHIC:
        cases += [("half_width 0", but(half_width=0.0)), ("half_height -1", but(half_height=-1.0)), ("half_width 2e30", but(half_width=2e30))]
    else:
        cases += [("lon_range 7", but(lon_range=7.0)), ("lat_range 3.2", but(lat_range=3.2)), ("lon_range 0", but(lon_range=0.0))]
    return cases


@pytest.mark.parametrize("kind", KINDS)
def test_every_refusal_leaves_the_next_frame_as_it_was(built, kind):
    from polaris_amd.tracer import HipTracer, TracerError

    W, H = FRAMES[0]
    sc, seeds = cornell(W, H), seeds_of()
    proj = image_projection(sc, kind)
    good = proj.params()
    lib = T.load_library()
    assert lib.polaris_hip_set_projection(None, C.byref(good)) == 2
    bare = HipTracer("bare", 0)
    bare.Init()
    try:
        assert lib.polaris_hip_set_projection(bare._h, C.byref(good)) == 2          # no camera set yet
        assert lib.polaris_hip_set_projection(bare._h, C.byref(T.projection_params())) == 0
    finally:
        bare.Close()
    tr = make_hip_tracer(sc, W, H)
    try:
        for state in ("off", "on"):
            if state == "on":
                tr.set_projection_params(good)
            before = frame_of(tr, request(W, H), seeds)
            assert lib.polaris_hip_set_projection(tr._h, None) == 2
            for what, p in refused_params(good):
                assert lib.polaris_hip_set_projection(tr._h, C.byref(p)) == 2, (state, what)
            if state == "on":                                                       # the lens and the shutter are refused while it is on
                with pytest.raises(TracerError, match="projection"):
                    tr.set_lens(0.05, 1.0)
                with pytest.raises(TracerError, match="projection"):
                    tr.set_shutter_params(T.shutter_params(sc.eye, sc.frustum))
                tr.set_lens(0.0)
                tr.set_shutter(None)
            after = frame_of(tr, request(W, H), seeds)
            assert before[1] == after[1] and np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[2], after[2]), state
        tr.set_projection(None)
        tr.set_lens(0.05, 1.0)                                                      # with the lens on the projection is refused
        with pytest.raises(TracerError, match="lens is on"):
            tr.set_projection_params(good)
        tr.set_lens(0.0)
        tr.set_projection_params(good)
    finally:
        tr.Close()


# ---- 7. temporal reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_prior_after_a_translation_is_the_host_restatements_and_the_history_follows_the_projection(built, host, kind, frame):
    W, H = frame
    spp = 3
    sc = cornell(W, H)
    proj = image_projection(sc, kind)
    step = F(0.05 * PO.scene_extent(sc))
    moved = dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + proj.right * step).astype(F))
    tr = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        tr.set_projection_params(proj.params())
        tr.set_temporal()
        trace(tr, W, H, spp, base=3, bounces=B)
        sync(tr, W, H, spp)
        hist, g0, a0 = tr.read_aov(T.AOV_TEMPORAL), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        # a translation of the eye: the history survives, PRIOR is the restatement's on the device's own planes
        set_cam(tr, moved)
        trace(tr, W, H, spp, base=5, bounces=B)
        sync(tr, W, H, spp)
        prior, g1, a1 = tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_GUIDE), tr.read_aov(T.AOV_ALBEDO)
        assert tr.kernel_symbol("reproject") == "pol::k_reproject_proj<false, false>"
        want = host.reproject_projection(hist, g0, a0, sc.eye, g1, a1, moved.eye, proj.params())
        assert np.array_equal(bits(prior), bits(want))
        assert (prior[..., 3] > 0).mean() > 0.1 and not np.array_equal(bits(g0), bits(g1))
        # a set_camera with the same eye: every filtered pixel takes history
        hist1 = tr.read_aov(T.AOV_TEMPORAL)
        set_cam(tr, moved)
        trace(tr, W, H, spp, base=7, bounces=B)
        sync(tr, W, H, spp)
        prior2 = tr.read_aov(T.AOV_PRIOR)
        filtered = GO.filtered_mask(a1)
        assert np.array_equal(prior2[..., 3] > 0, filtered) and filtered.sum() >= W * H // 8
        assert np.array_equal(bits(prior2), bits(host.reproject_projection(hist1, g1, a1, moved.eye, g1, a1, moved.eye, proj.params())))
        # an equal state keeps the history and the G-buffer: the planes are still readable and PRIOR is not recomputed
        tr.set_projection_params(proj.params())
        assert np.array_equal(bits(tr.read_aov(T.AOV_PRIOR)), bits(prior2))
        # a changed projection drops both: no PRIOR to read, the next sync starts without history, and the G-buffer is the new camera's
        other = PO.scene_projection(sc, kind, turned=False, **(PARTIAL if kind == PO.EQUIRECTANGULAR else {}))
        tr.set_projection_params(other.params())
        from polaris_amd.tracer import TracerError
        with pytest.raises(TracerError):
            tr.read_aov(T.AOV_PRIOR)
        g2 = tr.read_aov(T.AOV_GUIDE)
        assert not np.array_equal(bits(g2), bits(g1))
        trace(tr, W, H, spp, base=9, bounces=B)
        sync(tr, W, H, spp)
        assert not (tr.read_aov(T.AOV_PRIOR)[..., 3] > 0).any()
    finally:
        tr.Close()


# ---- 8. the layers above --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_hiptracer_set_projection_is_set_projection_params_with_the_derived_basis_and_follows_the_camera(built, kind):
    W, H = FRAMES[1]
    sc, seeds = cornell(W, H), seeds_of()
    height = PO.scene_extent(sc)
    args = dict(height=height) if kind == PO.ORTHOGRAPHIC else dict(lon_range=PARTIAL["lon_range"], lat_range=PARTIAL["lat_range"])
    name = "orthographic" if kind == PO.ORTHOGRAPHIC else "equirect"
    # a camera that looks another way: the frustum turned about the world's y axis
    c, s = np.cos(0.3), np.sin(0.3)
    fr = np.asarray(sc.frustum, np.float64).reshape(4, 4).copy()
    fr[:, 0], fr[:, 2] = c * fr[:, 0] + s * fr[:, 2], c * fr[:, 2] - s * fr[:, 0]
    turned = dataclasses.replace(sc, frustum=fr.astype(F).reshape(np.asarray(sc.frustum).shape))
    a, b = make_hip_tracer(sc, W, H), make_hip_tracer(turned, W, H)
    try:
        a.set_projection(name, **args)
        set_cam(a, turned)                                                          # the projection is re-sent with the new basis
        b.set_projection_params(T.projection_for(kind, turned.frustum, **args))
        fa, fb = frame_of(a, request(W, H), seeds), frame_of(b, request(W, H), seeds)
        assert fa[1] == fb[1] and np.array_equal(bits(fa[0]), bits(fb[0])) and np.array_equal(fa[2], fb[2]) and fa[0][..., :3].any()
        c_ = make_hip_tracer(sc, W, H)
        try:
            c_.set_projection(kind, **args)                                         # (by number, on the first camera: another image)
            fc = frame_of(c_, request(W, H), seeds)
        finally:
            c_.Close()
        assert not np.array_equal(bits(fc[0]), bits(fa[0]))
    finally:
        a.Close()
        b.Close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_host_layer_derives_the_same_projection(built, kind):
    from polaris_amd import host_api

    W, H = FRAMES[1]
    spp, bounces, rr = 3, 5, 3          # (the host renderer's defaults)
    sc0 = cornell(W, H)
    sc1 = cornell(W, H).set_camera(eye=(0.3, 0.55, -1.3), look=(0.55, 0.4, 0.2), fov=0.6911, aspect=W / H)   # turned: the basis changes
    args = dict(height=PO.scene_extent(sc0)) if kind == PO.ORTHOGRAPHIC else dict(lon_range=PARTIAL["lon_range"], lat_range=PARTIAL["lat_range"])
    seeds = seeds_of(spp, bounces, base=19)
    assert not np.array_equal(T.projection_from_frustum(sc1.frustum)[0], T.projection_from_frustum(sc0.frustum)[0])
    frames = []
    for raw in (False, True):
        tr = make_hip_tracer(sc0, W, H, exact_accumulate=1)
        try:
            if not raw:
                tr.set_projection(kind, **args)
            set_cam(tr, sc1)
            if raw:
                tr.set_projection_params(T.projection_for(kind, sc1.frustum, **args))
            tr.Trace(request(W, H, spp=spp, bounces=bounces, rr=rr), seeds)
            frames.append((tr.read_accumulator(0), counters(tr.last_trace_stats, bounces)))
        finally:
            tr.Close()
    assert frames[0][1] == frames[1][1] and np.array_equal(bits(frames[0][0]), bits(frames[1][0]))
    assert frames[0][0][..., :3].any()
    r = host_api.Renderer(sc0, [0], width=W, height=H, spp=spp, bounces=bounces, min_rr=rr, seed=3)
    try:
        r.set_option("exact_accumulate", 1)
        r.set_projection(kind, **args)
        r.set_camera(sc1.eye, sc1.frustum)      # (the projection stays on the camera, on the new basis)
        r.push_seeds(0, seeds)
        rows, _ = r.render()
        _, acc = r.read()
        with pytest.raises(RuntimeError, match="projection"):
            r.set_lens(0.05, 1.0)               # refused by the tracer while the projection is on
    finally:
        r.close()
    assert rows == [H]
    assert np.array_equal(bits(acc[..., :3]), bits(frames[0][0][..., :3]))


def test_render_cli_moves_a_panorama_with_temporal_reuse_as_the_frames_driven_by_hand(built, tmp_path):
    """--projection equirect --frames 2 --move right:0.05 --temporal 8: the two files are those of a Renderer given the same calls."""
    import subprocess
    import sys

    from conftest import ROOT
    from polaris_amd import host_api, render
    from test_gpu_denoise import ROOM_MTL, room_obj

    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    W, H, spp = 40, 20, 4
    flags = ["--projection", "equirect", "--lon-range", "120", "--lat-range", "60", "--frames", "2", "--move", "right:0.05", "--temporal", "8"]
    cmd = [sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--width", str(W), "--height", str(H), "--spp", str(spp),
           "--out", str(tmp_path / "cli.png")] + flags
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    cli = [open(p, "rb").read() for p in render.frame_paths(str(tmp_path / "cli.png"), 2)]
    sc = host_api.read_scene(str(tmp_path / "room.obj"), aspect=W / H)
    r = host_api.Renderer(sc, [0], width=W, height=H, spp=spp, bounces=5, min_rr=3, exposure=1.2, seed=1)
    by_hand = []
    try:
        r.set_temporal(max_history=8)
        r.set_projection("equirect", lon_range=np.radians(120.0), lat_range=np.radians(60.0))
        for k, path in enumerate(render.frame_paths(str(tmp_path / "hand.png"), 2)):
            eye, fr = host_api.camera_move(sc.camera, [render.parse_move("right:0.05")] * (k + 1), aspect=W / H)
            r.set_camera(eye, fr)
            r.render()
            r.save(path)
            by_hand.append(open(path, "rb").read())
        prior = r.read_aov(T.AOV_PRIOR)
    finally:
        r.close()
    assert cli == by_hand and cli[0] != cli[1]
    assert (prior[..., 3] > 0).any()            # the second frame took history across the move
    for bad_flags in (["--projection", "orthographic"], ["--projection", "equirect", "--aperture", "0.05", "--focus", "2"], ["--ortho-height", "2"]):
        bad = subprocess.run([sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj")] + bad_flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--projection" in bad.stderr      # (refused before the scene is read)
