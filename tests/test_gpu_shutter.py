"""The camera shutter on the MI355X (include/polaris_hip.h: polaris_hip_set_shutter).

Bars: with the shutter off a tracer is bit for bit the tracer that never heard of it, under the same kernel symbols; with it on,
polaris_hip_tap_primary's rays are tests/shutter_oracle.py's bit for bit and their hits the oracle's on those rays; a close state equal
to the open one gives the shutterless frame bit for bit through k_generate_shutter; the image does not depend on which traversal /
shade kernel family ran, on the origin width or on the batch size; on -> off -> on returns to the first frame; set_camera and a
changed set_lens switch the shutter off; every refusal leaves the state as it was; a changed shutter drops the temporal history and
identical bytes keep it; HipTracer.set_shutter, the C++ host layer and render.py --shutter send the same close state.

Frames: 24 x 10 rows [3, 9) (N = 144: one partly filled chunk) and 40 x 20 (N = 800: three full chunks and a tail); 3 spp, 3 bounces.
The close camera (shutter_oracle.close_camera): the open eye moved 0.05 x the scene's extent along TR - TL, the frustum turned 2
degrees about the up vector.
"""
import ctypes as C

import numpy as np
import pytest

import lens_oracle as LO
import shutter_oracle as SO
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_batched_exact import counters
from test_gpu_denoise import sync, trace
from test_gpu_lens import B, FRAMES, SPP, cornell, frame_of, moved, ray_scenes, request, scene_lens, seeds_of

pytestmark = pytest.mark.gpu

F = np.float32
E_BAD_ARGUMENT = 2
TAP_SEEDS = [7, 0x9E3779B9, 0xFFFFFFF0, 123456789]       # (0xFFFFFFF0: gx + seed wraps)
SYMBOL = {False: "pol::k_generate_shutter<false>", True: "pol::k_generate_shutter<true>"}
PULL = F(1.25)      # the close lens is focused this much further than the open one


class Cameras:
    """A scene's open lens and its close state: moved, turned, and under the lens focused PULL x further.  No entry is -0."""

    def __init__(self, sc):
        self.lens0, self.radius, self.focus = scene_lens(sc)
        self.eye1, self.frustum1 = SO.close_camera(sc)
        self.focus1 = F(self.focus * PULL)
        self.lens1 = LO.Lens.from_frustum(self.frustum1, self.radius, self.focus1)
        assert SO.no_negative_zero(sc.eye, sc.frustum, self.eye1, self.frustum1, *self.lens0.vectors()[1:], *self.lens1.vectors()[1:])

    def close(self):
        return SO.Close(self.eye1, self.frustum1, self.lens1)

    def params(self, lens: bool) -> T.ShutterParams:
        if not lens:
            return T.shutter_params(self.eye1, self.frustum1)
        return T.shutter_params(self.eye1, self.frustum1, *self.lens1.vectors())

    def apply(self, tr, lens: bool) -> None:
        """camera (set already), lens, shutter through the raw calls."""
        if lens:
            tr.set_lens_vectors(*self.lens0.vectors())
        tr.set_shutter_params(self.params(lens))


def same_as_open(sc, lens0=None) -> T.ShutterParams:
    if lens0 is None:
        return T.shutter_params(sc.eye, sc.frustum)
    return T.shutter_params(sc.eye, sc.frustum, *lens0.vectors())


def garbage_off() -> T.ShutterParams:
    """enabled = 0 with every float a NaN, an infinity or a huge number: nothing but `enabled` is looked at."""
    p = T.ShutterParams()
    words = (C.c_uint32 * 31).from_buffer(p)
    for k in range(2, 31):
        words[k] = (0x7FC00000, 0x7F800000, 0xFF800000, 0x7F7FFFFF)[k % 4]
    assert p.enabled == 0 and p.struct_size == 124
    return p


def same_frame(a, b) -> bool:
    return a[1] == b[1] and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2])


def raw_set_camera(tr, eye, frustum) -> int:
    e, f = np.ascontiguousarray(eye, F).reshape(3), np.ascontiguousarray(frustum, F).reshape(16)
    return tr._lib.polaris_hip_set_camera(tr._h, e.ctypes.data_as(C.POINTER(C.c_float)), f.ctypes.data_as(C.POINTER(C.c_float)))


# ---- 1. off is off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("lens", [False, True])
def test_a_shutter_that_is_off_is_the_tracer_that_never_heard_of_it(built, frame, exact, lens):
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    cams = Cameras(sc)
    got = []
    for off_shutter in (False, True):
        tr = make_hip_tracer(sc, W, H, exact_accumulate=exact, time_kernels=1)
        try:
            if lens:
                tr.set_lens_vectors(*cams.lens0.vectors())
            if off_shutter:
                tr.set_shutter_params(garbage_off())
                tr.set_shutter(None)
            got.append(frame_of(tr, request(W, H, by, bh), seeds) + (tr.kernel_symbol("generate"),))
        finally:
            tr.Close()
    assert got[0][3] == got[1][3] == ("pol::k_generate_lens" if lens else "pol::k_generate")
    assert same_frame(got[0], got[1]) and got[0][0][..., :3].any() and got[0][1][2] == W * bh * SPP


# ---- 2. ray bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["cornell", "moving-instances", "nested-shells"])
@pytest.mark.parametrize("lens", [False, True])
def test_tapped_rays_are_the_restatements_and_their_hits_the_oracles(built, oracle, name, frame, lens):
    W, H, by, bh = frame
    sc, options = ray_scenes(W, H)[name]
    cams = Cameras(sc)
    want = {}
    for seed in TAP_SEEDS:
        rays = SO.shutter_rays(oracle, sc, cams.close(), W, H, by, bh, seed, lens=cams.lens0 if lens else None)
        want[seed] = (rays,) + tuple(oracle.intersect(sc, rays))
    assert any(w[1].any() for w in want.values()), "no restated ray hits the scene"
    assert all((w[0][:, 0:3] != np.asarray(sc.eye, F)).any() for w in want.values()), "the shutter moved no origin"
    for packet in (0, 1):
        tr = make_hip_tracer(sc, W, H, packet_primary=packet, **options)
        try:
            cams.apply(tr, lens)
            for seed in TAP_SEEDS:
                taps = tr.tap_primary(request(W, H, by, bh), seed)
                rays, hit, wuvt, it = want[seed]
                what = (name, frame, lens, packet, seed)
                assert np.array_equal(bits(taps["primary_rays"]), bits(rays)), (what, int((bits(taps["primary_rays"]) != bits(rays)).sum()))
                assert np.array_equal(taps["primary_hit"] != 0, hit != 0), what
                h = hit != 0
                assert np.array_equal(bits(taps["primary_wuvt"][h]), bits(wuvt[h])), what
                assert np.array_equal(taps["primary_tri"][h], it[h]), what
        finally:
            tr.Close()


# ---- 3. close = open ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("lens", [False, True])
def test_a_close_state_equal_to_the_open_one_is_the_shutterless_frame(built, frame, exact, lens):
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    cams = Cameras(sc)
    got = []
    for shutter in (False, True):
        tr = make_hip_tracer(sc, W, H, exact_accumulate=exact, time_kernels=1)
        try:
            if lens:
                tr.set_lens_vectors(*cams.lens0.vectors())
            if shutter:
                tr.set_shutter_params(same_as_open(sc, cams.lens0 if lens else None))
            got.append(frame_of(tr, request(W, H, by, bh), seeds) + (tr.kernel_symbol("generate"),))
        finally:
            tr.Close()
    assert got[0][3] == ("pol::k_generate_lens" if lens else "pol::k_generate") and got[1][3] == SYMBOL[lens]
    assert same_frame(got[0], got[1]) and got[0][0][..., :3].any() and got[0][1][2] == W * bh * SPP


# ---- 4. one image whichever kernel ----------------------------------------------------------------------------------------------
def shutter_frame(sc, cams, lens, W, H, by, bh, seeds, **options):
    moments = options.pop("moments", 0)
    tr = make_hip_tracer(sc, W, H, **options)
    try:
        if moments:
            tr.set_option("moments", 1)
        cams.apply(tr, lens)
        tr.Trace(request(W, H, by, bh), seeds)
        return tr.read_accumulator(0), counters(tr.last_trace_stats, B)
    finally:
        tr.Close()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("lens", [False, True])
def test_one_image_whichever_kernel_traces_and_shades_it(built, frame, lens):
    """traversal x packet_primary x the node modes the Cornell box admits, with o12 and shade_wave going through their four
    combinations along the way, then the four on the default kernels; within exact and within batched mode."""
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    cams = Cameras(sc)
    grid = [dict(traversal=t, packet_primary=p, node_mode=n) for t in (1, 0) for p in (0, 1) for n in (2, 1, 0)]
    for exact in (1, 0):
        first = None
        for k, options in enumerate(grid):
            options = dict(options, o12=k & 1, shade_wave=(k >> 1) & 1, exact_accumulate=exact)
            acc, st = shutter_frame(sc, cams, lens, W, H, by, bh, seeds, **options)
            if first is None:
                first = (acc, st)
                assert acc[by:by + bh, :, :3].any() and st[2] == W * bh * SPP and st[4] > 0
            assert st == first[1], (exact, options)
            assert np.array_equal(bits(acc), bits(first[0])), (exact, options, int((bits(acc) != bits(first[0])).sum()))
        for o12, wave in ((0, 0), (0, 1), (1, 0), (1, 1)):
            acc, st = shutter_frame(sc, cams, lens, W, H, by, bh, seeds, exact_accumulate=exact, o12=o12, shade_wave=wave)
            assert st == first[1] and np.array_equal(bits(acc), bits(first[0])), (exact, o12, wave)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("lens", [False, True])
def test_batch_size_and_moments_do_not_change_the_shutter_image(built, frame, lens):
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    cams = Cameras(sc)
    ref, st = shutter_frame(sc, cams, lens, W, H, by, bh, seeds, samples_per_batch=1, overlap=3)
    assert not bits(ref[..., 3]).any()
    for options in (dict(samples_per_batch=2, overlap=2), dict(samples_per_batch=3), dict(samples_per_batch=2, overlap=2, moments=1), dict(moments=1)):
        acc, st2 = shutter_frame(sc, cams, lens, W, H, by, bh, seeds, **options)
        assert st2 == st, options
        assert np.array_equal(bits(acc[..., :3]), bits(ref[..., :3])), options
        assert bool(acc[by:by + bh, :, 3].any()) == bool(options.get("moments")), options


# ---- 5. switching on and off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("lens", [False, True])
def test_on_off_on_returns_to_the_first_frame(built, frame, lens):
    W, H, by, bh = frame
    sc, seeds = cornell(W, H), seeds_of()
    cams = Cameras(sc)
    plain = make_hip_tracer(sc, W, H, time_kernels=1)
    tr = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        if lens:
            plain.set_lens_vectors(*cams.lens0.vectors())
        shutterless = frame_of(plain, request(W, H, by, bh), seeds)
        cams.apply(tr, lens)
        first = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == SYMBOL[lens]
        tr.set_shutter(None)
        middle = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == ("pol::k_generate_lens" if lens else "pol::k_generate")
        tr.set_shutter_params(cams.params(lens))
        third = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == SYMBOL[lens]
    finally:
        plain.Close()
        tr.Close()
    assert same_frame(first, third) and same_frame(middle, shutterless)
    assert not np.array_equal(bits(first[0]), bits(shutterless[0]))      # (the shutter does something)


def test_set_camera_and_a_changed_lens_switch_the_shutter_off_and_an_identical_lens_keeps_it(built):
    W, H, by, bh = FRAMES[0]
    sc, seeds = cornell(W, H), seeds_of()
    sc1 = moved(sc, 0.02, 0.01)
    cams = Cameras(sc)
    focus2 = float(cams.focus) * 1.5
    fresh = {}
    for what in ("camera", "lens"):       # fresh tracers in the states the switched-off tracer must be in
        tr = make_hip_tracer(sc1 if what == "camera" else sc, W, H, time_kernels=1)
        try:
            tr.set_lens_vectors(*((cams.lens0.vectors()) if what == "camera" else (focus2,) + cams.lens0.vectors()[1:]))
            fresh[what] = frame_of(tr, request(W, H, by, bh), seeds)
            assert tr.kernel_symbol("generate") == "pol::k_generate_lens"
        finally:
            tr.Close()
    tr = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        cams.apply(tr, True)
        on = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == SYMBOL[True]
        tr.set_lens_vectors(*cams.lens0.vectors())                       # identical bytes: the shutter stays on
        again = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == SYMBOL[True] and same_frame(on, again)
        assert raw_set_camera(tr, sc1.eye, sc1.frustum) == 0             # the raw call: HipTracer re-applies nothing
        after_camera = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == "pol::k_generate_lens" and same_frame(after_camera, fresh["camera"])
        assert raw_set_camera(tr, sc.eye, sc.frustum) == 0
        tr.set_shutter_params(cams.params(True))
        back = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == SYMBOL[True] and same_frame(back, on)
        tr.set_lens_vectors(focus2, *cams.lens0.vectors()[1:])           # a changed byte: off
        after_lens = frame_of(tr, request(W, H, by, bh), seeds)
        assert tr.kernel_symbol("generate") == "pol::k_generate_lens" and same_frame(after_lens, fresh["lens"])
    finally:
        tr.Close()
    assert not same_frame(on, fresh["lens"]) and not same_frame(on, fresh["camera"])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def but(good, **kw):
    """A copy of the accepted `good` with these fields changed; name_i sets entry i of an array field."""
    p = T.ShutterParams()
    C.memmove(C.byref(p), C.byref(good), C.sizeof(p))
    for k, v in kw.items():
        if k in ("struct_size", "enabled", "focus_distance1"):
            setattr(p, k, v)
        else:
            name, i = k.rsplit("_", 1)
            getattr(p, name)[int(i)] = v
    return p


def refused_always(good):
    cases = [(f"struct_size {n}", but(good, struct_size=n)) for n in (0, 120, 128, 44)]
    cases += [(f"enabled {n}", but(good, enabled=n)) for n in (2, 0xFFFFFFFF)]
    for k in range(19):                                                   # each of the 19 camera floats
        field = f"eye1_{k}" if k < 3 else f"frustum1_{k - 3}"
        for bad in (float("nan"), float("inf"), float("-inf")):
            cases.append((f"{field} = {bad}", but(good, **{field: bad})))
    return cases


def refused_under_a_lens(good):
    """set_lens' own rules for the close lens, each one field away from the accepted `good`."""
    cases = []
    for field in ("focus_distance1", "axis1_0", "axis1_2", "u1_0", "u1_2", "v1_1"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            cases.append((f"{field} = {bad}", but(good, **{field: bad})))
    cases += [("u1 above 2^30", but(good, u1_1=2.0 ** 30 * 1.001)), ("v1 below -2^30", but(good, v1_2=-2.0 ** 31))]
    cases += [(f"focus_distance1 {d}", but(good, focus_distance1=d)) for d in (0.0, -1.0, 0.99e-6, 1.01e30)]
    cases += [("short axis1", but(good, axis1_0=0.0, axis1_1=0.0, axis1_2=0.9985)), ("long axis1", but(good, axis1_0=0.0, axis1_1=0.0, axis1_2=1.0015)),
              ("zero axis1", but(good, axis1_0=0.0, axis1_1=0.0, axis1_2=0.0))]
    return cases


def test_every_refusal_leaves_the_state_as_it_was(built):
    from polaris_amd.tracer import HipTracer

    W, H, by, bh = FRAMES[0]
    sc, seeds = cornell(W, H), seeds_of()
    cams = Cameras(sc)
    bare = HipTracer("no camera", 0)
    bare.Init()
    try:
        for p in (cams.params(False), T.shutter_params()):
            assert bare._lib.polaris_hip_set_shutter(bare._h, C.byref(p)) == E_BAD_ARGUMENT      # no camera set yet
            assert b"set_shutter" in bare._lib.polaris_hip_last_error(bare._h)
    finally:
        bare.Close()
    tr = make_hip_tracer(sc, W, H, time_kernels=1)
    try:
        lib, h = tr._lib, tr._h
        assert lib.polaris_hip_set_shutter(None, C.byref(cams.params(False))) == E_BAD_ARGUMENT
        for lens in (False, True):
            if lens:
                tr.set_lens_vectors(*cams.lens0.vectors())
            good = cams.params(lens)
            refused = refused_always(good) + (refused_under_a_lens(good) if lens else [])
            for state in ("off", "on"):
                if state == "on":
                    assert lib.polaris_hip_set_shutter(h, C.byref(good)) == 0
                before = frame_of(tr, request(W, H, by, bh), seeds)
                symbol = tr.kernel_symbol("generate")
                assert symbol == (SYMBOL[lens] if state == "on" else ("pol::k_generate_lens" if lens else "pol::k_generate"))
                assert lib.polaris_hip_set_shutter(h, None) == E_BAD_ARGUMENT
                for what, p in refused:
                    assert lib.polaris_hip_set_shutter(h, C.byref(p)) == E_BAD_ARGUMENT, (lens, state, what)
                    assert b"set_shutter" in lib.polaris_hip_last_error(h), (lens, state, what)
                    after = frame_of(tr, request(W, H, by, bh), seeds)      # the next frame after each refusal
                    assert same_frame(before, after) and tr.kernel_symbol("generate") == symbol, (lens, state, what)
            if not lens:      # with the lens off the ten lens floats are not looked at
                for what, p in refused_under_a_lens(good):
                    assert lib.polaris_hip_set_shutter(h, C.byref(p)) == 0, what
            else:             # accepted at the edges of the ranges, and with the aperture closing over the interval
                for p in (but(good, focus_distance1=1e-6), but(good, focus_distance1=1e30), but(good, u1_0=2.0 ** 30, v1_1=-2.0 ** 30),
                          but(good, u1_0=0.0, u1_1=0.0, u1_2=0.0, v1_0=0.0, v1_1=0.0, v1_2=0.0)):
                    assert lib.polaris_hip_set_shutter(h, C.byref(p)) == 0
            assert lib.polaris_hip_set_shutter(h, C.byref(T.shutter_params())) == 0
    finally:
        tr.Close()


# ---- 7. history -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", [True, False])
def test_a_changed_shutter_drops_the_temporal_history_and_identical_bytes_keep_it(built, change):
    """(A history is captured at a camera move, and set_camera switches the shutter off: the history under test is one seen with the
    shutter off, and the identical bytes are those of another off state.)"""
    W, H, spp = 40, 20, 2
    sc0 = cornell(W, H)
    sc1 = moved(sc0, 0.02, 0.01)        # (the eye alone moves)
    cams = Cameras(sc1)
    tr = make_hip_tracer(sc0, W, H, time_kernels=1)
    try:
        tr.set_temporal()
        trace(tr, W, H, spp, base=3, bounces=B)
        sync(tr, W, H, spp)
        guide = tr.read_aov(T.AOV_GUIDE)
        assert raw_set_camera(tr, sc1.eye, sc1.frustum) == 0
        trace(tr, W, H, spp, base=5, bounces=B)
        sync(tr, W, H, spp)
        prior, guide1 = tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_GUIDE)
        assert (prior[..., 3] > 0).any()                              # the second sync found the first view's history (not vacuous)
        tr.set_shutter_params(cams.params(False) if change else garbage_off())      # (any two off states are equal)
        trace(tr, W, H, spp, base=7, bounces=B)
        assert tr.kernel_symbol("generate") == (SYMBOL[False] if change else "pol::k_generate")
        sync(tr, W, H, spp)
        after, guide2 = tr.read_aov(T.AOV_PRIOR), tr.read_aov(T.AOV_GUIDE)
    finally:
        tr.Close()
    assert np.array_equal(bits(guide1), bits(guide2)) and not np.array_equal(bits(guide), bits(guide1))   # the guide is the open pinhole's, shutter or not
    if change:
        assert not after[..., 3].any()
    else:
        assert np.array_equal(bits(after), bits(prior))


# ---- 8. the layers above --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True])
def test_set_shutter_and_the_host_layer_send_the_raw_calls_close_state(built, lens):
    from polaris_amd import host_api
    from polaris_amd.tracer import ChangeType, UpdateMode

    W, H, by, bh = FRAMES[1]
    spp, bounces, rr = 3, 5, 3          # (the host renderer's defaults)
    sc = cornell(W, H)
    cams = Cameras(sc)
    seeds = seeds_of(spp, bounces, base=19)
    frames = []
    for how in ("raw", "set_shutter", "lens after"):
        tr = make_hip_tracer(sc, W, H, exact_accumulate=1, time_kernels=1)
        try:
            if how == "raw":
                cams.apply(tr, lens)
            elif how == "set_shutter":
                if lens:
                    tr.set_lens(cams.radius, cams.focus)
                tr.set_shutter(cams.eye1, cams.frustum1, cams.focus1 if lens else None)
            else:                        # the shutter first, then the lens: set_lens re-sends the shutter with the new close lens
                tr.set_shutter(cams.eye1, cams.frustum1, cams.focus1 if lens else None)
                if lens:
                    tr.set_lens(cams.radius, cams.focus)
            req = request(W, H, by, bh, spp=spp, bounces=bounces, rr=rr)
            tr.Trace(req, seeds)
            assert tr.kernel_symbol("generate") == SYMBOL[lens], how
            frames.append((tr.read_accumulator(0), counters(tr.last_trace_stats, bounces)))
            if how == "set_shutter":     # a camera update forgets the shutter: the library has switched it off
                tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)
                tr.Trace(request(W, H, by, bh, spp=spp, bounces=bounces, rr=rr), seeds)
                assert tr.kernel_symbol("generate") == ("pol::k_generate_lens" if lens else "pol::k_generate")
                assert tr._shutter is None
        finally:
            tr.Close()
    for other in frames[1:]:
        assert frames[0][1] == other[1] and np.array_equal(bits(frames[0][0]), bits(other[0]))
    assert frames[0][0][..., :3].any()
    r = host_api.Renderer(sc, [0], width=W, height=H, spp=spp, bounces=bounces, min_rr=rr, seed=3)
    try:
        r.set_option("exact_accumulate", 1)
        if lens:
            r.set_lens(cams.radius, cams.focus)
        r.set_shutter(cams.eye1, cams.frustum1, cams.focus1 if lens else None)
        r.push_seeds(0, seeds)
        rows, _ = r.render()
        _, acc = r.read()
        r.set_camera(sc.eye, sc.frustum)        # (drops the close state)
        r.push_seeds(0, seeds)
        r.render()
        _, acc_open = r.read()
    finally:
        r.close()
    assert rows == [H]
    assert np.array_equal(bits(acc[..., :3]), bits(frames[0][0][..., :3]))
    assert not np.array_equal(bits(acc_open[..., :3]), bits(acc[..., :3]))


def test_render_cli_shutter_frames_match_the_renderer_driven_by_hand(built, tmp_path):
    """--frames 2 --shutter 0.5: frame k's shutter closes at the camera after k + 1 moves and one more of half the offset."""
    import subprocess
    import sys

    from conftest import ROOT
    from polaris_amd import host_api
    from test_gpu_denoise import ROOM_MTL, room_obj

    (tmp_path / "room.obj").write_text(room_obj())
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    W, H = 40, 20
    base = [sys.executable, "-m", "polaris_amd.render", str(tmp_path / "room.obj"), "--width", str(W), "--height", str(H), "--spp", "4",
            "--frames", "2", "--move", "right:0.2", "--aperture", "0.05", "--focus", "3.0"]
    for name, flags in (("s.png", ["--shutter", "0.5"]), ("p.png", [])):
        r = subprocess.run(base + flags + ["--out", str(tmp_path / name)], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    sc = host_api.read_scene(str(tmp_path / "room.obj"), aspect=W / H)
    rd = host_api.Renderer(sc, [0], width=W, height=H, spp=4, bounces=5, min_rr=3, exposure=1.2, seed=1)
    try:
        rd.set_lens(0.05, 3.0)
        for k in range(2):
            rd.set_camera(*host_api.camera_move(sc.camera, [("right", 0.2)] * (k + 1), aspect=W / H))
            rd.set_shutter(*host_api.camera_move(sc.camera, [("right", 0.2)] * (k + 1) + [("right", 0.1)], aspect=W / H))
            rd.render(0)
            rd.save(str(tmp_path / f"hand_{k}.png"))
    finally:
        rd.close()
    for k in range(2):
        shuttered, plain = open(tmp_path / f"s_{k:03d}.png", "rb").read(), open(tmp_path / f"p_{k:03d}.png", "rb").read()
        assert shuttered == open(tmp_path / f"hand_{k}.png", "rb").read() and shuttered != plain, k
