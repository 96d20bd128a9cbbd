"""The thin-lens camera on the MI355X (include/polaris_hip.h: polaris_hip_set_lens).

Bars: with the lens off a tracer is bit for bit the tracer that never heard of it, under the same kernel symbol; with it on,
polaris_hip_tap_primary's rays are tests/lens_oracle.py's bit for bit and their hits the oracle's on those rays; the image does not
depend on which traversal / shade kernel family ran, on the origin width or on the batch size; on -> off -> on returns to the first
frame through the pinhole's; every refusal leaves the state as it was; a changed lens drops the temporal history and identical bytes
keep it; HipTracer.set_lens follows the camera, and the C++ host layer derives the same lens; render.py's --focus-pixel is --focus
at the distance the GUIDE plane gives.

Frames: 24 x 10 rows [3, 9) (N = 144: one partly filled chunk) and 40 x 20 (N = 800: three full chunks and a tail).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lens_oracle as LO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_batched_exact import counters
from test_gpu_denoise import sync, trace
from test_gpu_parity import _nested_shells_scene

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES = [(24, 10, 3, 6), (40, 20, 0, 20)]      # W, H, block_y, block_h
SPP, B, RR = 3, 3, 1
E_BAD_ARGUMENT = 2


def request(W, H, by, bh, spp=SPP, bounces=B, rr=RR):
    from oracle import pybind as ob

    return ob.make_request(W, H, spp=spp, bounces=bounces, rr=rr, block_y=by, block_h=bh)


def seeds_of(spp=SPP, bounces=B, base=41):
    from polaris_amd import scenes

    return scenes.make_seeds(spp, bounces, base=base)


def scene_lens(sc, radius_of_extent=0.05):
    """A round lens of 0.05 x the scene's extent, focused on the middle of the scene's box along the view axis."""
    lo, hi = sc.bvh_nodes["min"].min(axis=0).astype(np.float64), sc.bvh_nodes["max"].max(axis=0).astype(np.float64)
    radius = F(radius_of_extent * float((hi - lo).max()))
    axis = T.lens_from_frustum(sc.frustum, radius)[0].astype(np.float64)
    focus = max(float(np.dot((lo + hi) / 2 - np.asarray(sc.eye, np.float64), axis)), 0.25 * float((hi - lo).max()))
    return LO.Lens.from_frustum(sc.frustum, radius, F(focus)), radius, F(focus)


def cornell(W, H):
    from polaris_amd import scenes

    return scenes.SCENES["cornell"](W / H)


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
@pytest.mark.parametrize("exact", [1, 0])
def test_an_all_zero_lens_is_the_tracer_that_never_heard_of_it(built, frame, exact):
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    got = []
    for zero_lens in (False, True):
        tr = make_hip_tracer(sc, W, H, exact_accumulate=exact, time_kernels=1)
        try:
            if zero_lens:
                tr.set_lens_vectors(3.0, (0, 0, 1), (0, 0, 0), (0, 0, 0))    # u = v = 0: off, nothing else is looked at
                tr.set_lens(0.0)
            got.append(frame_of(tr, request(W, H, by, bh), seeds) + (tr.kernel_symbol("generate"),))
        finally:
            tr.Close()
    (acc_a, st_a, fb_a, sym_a), (acc_b, st_b, fb_b, sym_b) = got
    assert sym_a == sym_b == "pol::k_generate"
    assert st_a == st_b and st_a[2] == W * bh * SPP
    assert np.array_equal(bits(acc_a), bits(acc_b)) and acc_a[..., :3].any()
    assert np.array_equal(fb_a, fb_b)


# ---- 2. ray bits ----------------------------------------------------------------------------------------------------------------
def ray_scenes(W, H):
    from polaris_amd import scenes

    return {"cornell": (cornell(W, H), {}),                                                       # tiny-scene mode
            "moving-instances": (scenes.moving_instances(0, W / H), {}),
            "nested-shells": (_nested_shells_scene(), {"node_mode": 0, "max_leaf_tris": 0})}      # the tree stays in HBM, 24-entry stack


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["cornell", "moving-instances", "nested-shells"])
def test_tapped_rays_are_the_restatements_and_their_hits_the_oracles(built, oracle, name, frame):
    W, H, by, bh = frame
    sc, options = ray_scenes(W, H)[name]
    lens, radius, focus = scene_lens(sc)
    tap_seeds = [7, 0x9E3779B9, 0xFFFFFFF0, 123456789]       # (0xFFFFFFF0: gx + seed wraps)
    want = {}
    for seed in tap_seeds:
        rays = LO.lens_rays(oracle, sc, lens, W, H, by, bh, seed)
        want[seed] = (rays,) + tuple(oracle.intersect(sc, rays))
    assert any(w[1].any() for w in want.values()), "no restated ray hits the scene"
    assert any((w[0][:, 0:3] != np.asarray(sc.eye, F)).any() for w in want.values()), "the lens moved no origin"
    for packet in (0, 1):
        tr = make_hip_tracer(sc, W, H, packet_primary=packet, **options)
        try:
            tr.set_lens(radius, focus)
            for seed in tap_seeds:
                taps = tr.tap_primary(request(W, H, by, bh), seed)
                rays, hit, wuvt, it = want[seed]
                what = (name, frame, packet, seed)
                assert np.array_equal(bits(taps["primary_rays"]), bits(rays)), (what, int((bits(taps["primary_rays"]) != bits(rays)).sum()))
                assert np.array_equal(taps["primary_hit"] != 0, hit != 0), what
                h = hit != 0
                assert np.array_equal(bits(taps["primary_wuvt"][h]), bits(wuvt[h])), what
                assert np.array_equal(taps["primary_tri"][h], it[h]), what
        finally:
            tr.Close()


# ---- 3. one image whichever kernel ----------------------------------------------------------------------------------------------
def lens_frame(sc, W, H, by, bh, lens_args, seeds, spp=SPP, **options):
    moments = options.pop("moments", 0)
    tr = make_hip_tracer(sc, W, H, **options)
    try:
        if moments:
            tr.set_option("moments", 1)
        tr.set_lens(*lens_args)
        req = request(W, H, by, bh, spp=spp)
        tr.Trace(req, seeds)
        return tr.read_accumulator(0), counters(tr.last_trace_stats, B)
    finally:
        tr.Close()


@pytest.mark.parametrize("frame", FRAMES)
def test_one_image_whichever_kernel_traces_and_shades_it(built, frame):
    """traversal x packet_primary x the node modes the Cornell box admits (records in global memory, the tree's top in LDS, the
    tiny-scene mode), with o12 and shade_wave going through their four combinations along the way."""
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    _, radius, focus = scene_lens(sc)
    grid = [dict(traversal=t, packet_primary=p, node_mode=n) for t in (1, 0) for p in (0, 1) for n in (2, 1, 0)]
    for exact in (1, 0):
        first = None
        for k, options in enumerate(grid):
            options = dict(options, o12=k & 1, shade_wave=(k >> 1) & 1, exact_accumulate=exact)
            acc, st = lens_frame(sc, W, H, by, bh, (radius, focus), seeds, **options)
            if first is None:
                first = (acc, st)
                assert acc[by:by + bh, :, :3].any() and st[2] == W * bh * SPP and st[4] > 0
            assert st == first[1], (exact, options)
            assert np.array_equal(bits(acc), bits(first[0])), (exact, options, int((bits(acc) != bits(first[0])).sum()))
    # the remaining o12 / shade_wave combinations on the default kernels
    for exact in (1, 0):
        ref = lens_frame(sc, W, H, by, bh, (radius, focus), seeds, exact_accumulate=exact)
        for o12, wave in ((0, 0), (0, 1), (1, 0), (1, 1)):
            acc, st = lens_frame(sc, W, H, by, bh, (radius, focus), seeds, exact_accumulate=exact, o12=o12, shade_wave=wave)
            assert st == ref[1] and np.array_equal(bits(acc), bits(ref[0])), (exact, o12, wave)


@pytest.mark.parametrize("frame", FRAMES)
def test_batch_size_and_moments_do_not_change_the_lens_image(built, frame):
    """The batched accumulator is the per-sample sum whatever samples_per_batch is (tests/test_gpu_batched_exact.py pins that for
    the pinhole camera: every batch size equals one reference, so they equal each other); "moments" adds .w and leaves .rgb."""
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    _, radius, focus = scene_lens(sc)
    ref, st = lens_frame(sc, W, H, by, bh, (radius, focus), seeds, samples_per_batch=1, overlap=3)
    assert not bits(ref[..., 3]).any()
    for options in (dict(samples_per_batch=2, overlap=2), dict(samples_per_batch=3), dict(samples_per_batch=2, overlap=2, moments=1), dict(moments=1)):
        acc, st2 = lens_frame(sc, W, H, by, bh, (radius, focus), seeds, **options)
        assert st2 == st, options
        assert np.array_equal(bits(acc[..., :3]), bits(ref[..., :3])), options
        assert bool(acc[by:by + bh, :, 3].any()) == bool(options.get("moments")), options


# ---- 4. a bounded sequence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
def test_on_off_on_returns_to_the_first_frame_through_the_pinholes(built, frame):
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    _, radius, focus = scene_lens(sc)
    pin = make_hip_tracer(sc, W, H, time_kernels=1)
    tr = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        pinhole = frame_of(pin, request(W, H, by, bh), seeds)
        tr.set_lens(radius, focus)
        first = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == "pol::k_generate_lens"
        tr.set_lens(0.0)
        middle = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == "pol::k_generate"
        tr.set_lens(radius, focus)
        third = frame_of(tr, request(W, H, by, bh), seeds)
    finally:
        pin.Close()
        tr.Close()
    for a, b, what in ((first, third, "first / third"), (middle, pinhole, "middle / pinhole")):
        assert a[1] == b[1], what
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2]), what
    assert not np.array_equal(bits(first[0]), bits(pinhole[0]))      # (the lens does something)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def refused_params(good):
    """(what, params) of every refusal include/polaris_hip.h lists, each one field away from the accepted `good`."""
    def but(**kw):
        p = T.LensParams()
        C.memmove(C.byref(p), C.byref(good), C.sizeof(p))
        for k, v in kw.items():
            if k == "struct_size":
                p.struct_size = v
            elif k == "focus_distance":
                p.focus_distance = v
            else:
                name, i = k.split("_")
                getattr(p, name)[int(i)] = v
        return p

    cases = [("struct_size 40", but(struct_size=40)), ("struct_size 48", but(struct_size=48)), ("struct_size 0", but(struct_size=0))]
    for field in ("focus_distance", "axis_0", "axis_2", "u_0", "u_2", "v_1"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            cases.append((f"{field} = {bad}", but(**{field: bad})))
    cases += [("u above 2^30", but(u_1=2.0 ** 30 * 1.001)), ("v below -2^30", but(v_2=-2.0 ** 31))]
    cases += [(f"focus_distance {d}", but(focus_distance=d)) for d in (0.0, -1.0, 0.99e-6, 1.01e30)]
    cases += [("short axis", but(axis_0=0.0, axis_1=0.0, axis_2=0.9985)),     # squared 0.9970
              ("long axis", but(axis_0=0.0, axis_1=0.0, axis_2=1.0015)),      # squared 1.0030
              ("zero axis", but(axis_0=0.0, axis_1=0.0, axis_2=0.0))]
    return cases


def test_every_refusal_leaves_the_state_as_it_was(built):
    W, H, by, bh = FRAMES[0]
    sc, seeds = cornell(W, H), seeds_of()
    lens, radius, focus = scene_lens(sc)
    good = T.lens_params(*lens.vectors())
    tr = make_hip_tracer(sc, W, H)
    try:
        lib, h = tr._lib, tr._h
        assert lib.polaris_hip_set_lens(None, C.byref(good)) == E_BAD_ARGUMENT
        for state in ("off", "on"):
            if state == "on":
                assert lib.polaris_hip_set_lens(h, C.byref(good)) == 0
            before = frame_of(tr, request(W, H, by, bh), seeds)
            assert lib.polaris_hip_set_lens(h, None) == E_BAD_ARGUMENT
            for what, p in refused_params(good):
                assert lib.polaris_hip_set_lens(h, C.byref(p)) == E_BAD_ARGUMENT, (state, what)
                assert b"set_lens" in lib.polaris_hip_last_error(h), (state, what)
            after = frame_of(tr, request(W, H, by, bh), seeds)
            assert before[1] == after[1] and np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[2], after[2]), state
        # accepted at the edges of the ranges, and with the lens off whatever focus and axis say
        for p in (T.lens_params(1e-6, lens.axis, lens.u, lens.v), T.lens_params(1e30, lens.axis, lens.u, lens.v),
                  T.lens_params(focus, lens.axis, (2.0 ** 30, 0, 0), (0, -2.0 ** 30, 0)), T.lens_params(-5.0, (0, 0, 0), (0, 0, 0), (0, 0, 0))):
            assert lib.polaris_hip_set_lens(h, C.byref(p)) == 0
    finally:
        tr.Close()


# ---- 6. history -----------------------------------------------------------------------------------------------------------------
def moved(sc, dx, dy=0.0):
    return dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([dx, dy, 0], F)).astype(F))


@pytest.mark.parametrize("change", [True, False])
def test_a_changed_lens_drops_the_temporal_history_and_identical_bytes_keep_it(built, change):
    from polaris_amd.tracer import ChangeType, UpdateMode

    W, H, spp = 40, 20, 2
    sc0 = cornell(W, H)
    sc1 = moved(sc0, 0.02, 0.01)        # (the eye alone moves: the frustum, and with it the lens vectors, stay)
    lens, radius, focus = scene_lens(sc0)
    tr = make_hip_tracer(sc0, W, H)
    try:
        tr.set_temporal()
        tr.set_lens_vectors(*lens.vectors())
        trace(tr, W, H, spp, base=3, bounces=B)
        sync(tr, W, H, spp)
        guide = tr.read_aov(T.AOV_GUIDE)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc1)
        trace(tr, W, H, spp, base=5, bounces=B)
        sync(tr, W, H, spp)
        prior, guide1 = tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_GUIDE)
        assert (prior[..., 3] > 0).any()                              # the second sync found the first view's history (not vacuous)
        if change:
            tr.set_lens_vectors(float(focus) * 1.5, lens.axis, lens.u, lens.v)
        else:
            tr.set_lens_vectors(*lens.vectors())
        trace(tr, W, H, spp, base=7, bounces=B)
        sync(tr, W, H, spp)
        after, guide2 = tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    assert np.array_equal(bits(guide1), bits(guide2)) and not np.array_equal(bits(guide), bits(guide1))   # the guide is the pinhole's, lens or not
    if change:
        assert not after[..., 3].any()
    else:
        assert np.array_equal(bits(after), bits(prior))


# ---- 7. the layers above --------------------------------------------------------------------------------------------------------
def test_set_lens_follows_the_camera_and_the_host_layer_derives_the_same_lens(built):
    from polaris_amd import host_api, scenes
    from polaris_amd.tracer import ChangeType, UpdateMode

    W, H, by, bh = FRAMES[1]
    spp, bounces, rr = 3, 5, 3          # (the host renderer's defaults)
    sc0 = cornell(W, H)
    sc1 = cornell(W, H).set_camera(eye=(0.3, 0.55, -1.3), look=(0.55, 0.4, 0.2), fov=0.6911, aspect=W / H)   # turned: the lens vectors change
    _, radius, focus = scene_lens(sc0)
    seeds = seeds_of(spp, bounces, base=19)
    axis, u, v = T.lens_from_frustum(sc1.frustum, radius)
    assert not np.array_equal(axis, T.lens_from_frustum(sc0.frustum, radius)[0])
    frames = []
    for raw in (False, True):
        tr = make_hip_tracer(sc0, W, H, exact_accumulate=1)
        try:
            if not raw:
                tr.set_lens(radius, focus)
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc1)
            if raw:
                tr.set_lens_vectors(focus, axis, u, v)
            req = request(W, H, by, bh, spp=spp, bounces=bounces, rr=rr)
            tr.Trace(req, seeds)
            frames.append((tr.read_accumulator(0), counters(tr.last_trace_stats, bounces)))
        finally:
            tr.Close()
    assert frames[0][1] == frames[1][1] and np.array_equal(bits(frames[0][0]), bits(frames[1][0]))
    assert frames[0][0][..., :3].any()
    r = host_api.Renderer(sc0, [0], width=W, height=H, spp=spp, bounces=bounces, min_rr=rr, seed=3)
    try:
        r.set_option("exact_accumulate", 1)
        r.set_lens(radius, focus)
        r.set_camera(sc1.eye, sc1.frustum)      # (the lens stays on the camera)
        r.push_seeds(0, seeds)
        rows, _ = r.render()
        _, acc = r.read()
    finally:
        r.close()
    assert rows == [H]
    assert np.array_equal(bits(acc[..., :3]), bits(frames[0][0][..., :3]))


def test_render_cli_focuses_on_what_a_pixel_sees(built, tmp_path):
    """--aperture with --focus-pixel: the frame of --focus D with D = t * dot(centre direction, axis) from the GUIDE plane, and not the pinhole's."""
    import subprocess
    import sys

    from conftest import ROOT
    from polaris_amd import host_api, render
    from test_gpu_denoise import ROOM_MTL, room_obj

    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    W, H = 40, 20
    sc = host_api.read_scene(str(tmp_path / "room.obj"), aspect=W / H)
    tr = make_hip_tracer(sc, W, H)
    try:
        focus = render.focus_of_pixel(tr.read_aov(T.AOV_GUIDE), sc.frustum, 13, 15)
    finally:
        tr.Close()
    assert 2.0 < focus < 4.5          # the eye stands 2.4 in front of the room, which is 2 deep

    def frame(name, *flags):
        cmd = [sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--width", str(W), "--height", str(H), "--spp", "4",
               "--out", str(tmp_path / name)] + list(flags)
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(tmp_path / name, "rb").read()

    by_pixel = frame("pixel.png", "--aperture", "0.05", "--focus-pixel", "13,15")
    by_distance = frame("distance.png", "--aperture", "0.05", "--focus", repr(focus))
    pinhole = frame("pinhole.png")
    assert by_pixel == by_distance and by_pixel != pinhole
    bad = subprocess.run([sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--aperture", "0.05"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--focus" in bad.stderr      # (refused before the scene is read)
