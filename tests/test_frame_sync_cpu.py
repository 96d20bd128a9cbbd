"""CPU test of the rules behind polaris_hip_sync_framebuffer's planes (polaris_amd/csrc/frame_sync.h): what of the lazily allocated
planes is valid after every event, which planes an event frees or swaps into the history, what a sync with the features in force
does, and which AOVs polaris_hip_read_aov hands out or refuses, with which words.

tests/tools/frame_sync_check.cpp hands plain numbers to the header.  Every expectation below is written out by hand from DESIGN.md
sections 10-10d and the host code before the header existed; none is read back from the library.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "frame_sync_check.cpp")
LIB = os.path.join(BUILD, "libframe_sync_check.so")

PLANES = ["guide", "albedo", "denoised", "temporal", "prior", "variance", "prior2", "ping", "pong", "hist", "hguide", "halbedo", "vhist",
          "inst", "hinst", "motion_table"]
AOV_NAMES = PLANES[:7]                       # POLARIS_AOV_GUIDE .. POLARIS_AOV_PRIOR2 = 0 .. 6
DENOISE, TEMPORAL, VARIANCE, MOTION = 1, 2, 4, 8
(RESIZED, CAMERA_MOVED, SCENE_CHANGED, TEMPORAL_PARAMS_CHANGED, TEMPORAL_OFF, VARIANCE_TOGGLED, MOTION_TOGGLED, GBUFFER_COMPUTED, PRIOR_COMPUTED,
 SYNCED) = range(10)
GBUFFER, PRIOR, HAVE_HISTORY, HISTORY_M2, TEMPORAL_SYNCED, VARIANCE_SYNCED = 1, 2, 4, 8, 16, 32
ACCUMULATOR, TEMPORAL_PLANE, DENOISED_PLANE = 0, 1, 2                            # SyncSource
NO_TABLE, TABLE, MOVED, OTHER_MESH, READ_BACK, OPTION_OFF = range(6)             # frame_sync_check.cpp table_of

NO_DENOISED = "read_aov: no denoised sync since the last resize"
NO_TEMPORAL = "read_aov: no temporal sync under the current camera"
NO_VARIANCE_CAMERA = "read_aov: no variance sync under the current camera"
NO_VARIANCE_RESIZE = "read_aov: no variance sync since the last resize"
NO_PRIOR2 = "read_aov: no variance sync with temporal reuse under the current camera"


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "frame_sync.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    so.frame_sync_new.restype = C.c_void_p
    so.frame_sync_delete.restype = None
    for name in ("frame_sync_event", "frame_sync_flags", "frame_sync_table", "frame_sync_plane_sets"):
        getattr(so, name).restype = C.c_int64
    so.frame_sync_aov_refusal.restype = C.c_char_p
    so.frame_sync_step_timer.restype = C.c_char_p
    so.frame_sync_plan.restype = None
    so.frame_sync_set_current_table.restype = None
    return so


def mask(*names):
    return sum(1 << PLANES.index(n) for n in names)


def names(bits):
    assert bits >> len(PLANES) == 0
    return {n for i, n in enumerate(PLANES) if bits >> i & 1}


class State:
    """A SyncState, and beside it what the owner of the planes does with the sets the transitions return: `planes` is the set of
    planes that exist.  sync() and read_gbuffer() fire the events of polaris_hip_sync_framebuffer and of read_aov(GUIDE)."""

    def __init__(self, lib):
        self.lib, self.s, self.features, self.planes = lib, C.c_void_p(lib.frame_sync_new()), 0, set()

    def close(self):
        self.lib.frame_sync_delete(self.s)

    def event(self, event, arg=0):
        return self.lib.frame_sync_event(self.s, C.c_int64(event), C.c_int64(self.features), C.c_int64(arg))

    def flags(self):
        return self.lib.frame_sync_flags(self.s)

    def tables(self):
        return (self.lib.frame_sync_table(self.s, C.c_int64(0)), self.lib.frame_sync_table(self.s, C.c_int64(1)))

    def plan(self, features=None):
        out = (C.c_int64 * 14)()
        self.lib.frame_sync_plan(self.s, C.c_int64(self.features if features is None else features), out)
        need, clear, clear_new, prior, history, m2, motion, color, tonemap, n = out[:10]
        steps = [self.lib.frame_sync_step_timer(C.c_int64(s)).decode() for s in out[10:10 + n]]
        assert list(out[10 + n:]) == [-1] * (4 - n)
        return dict(need=names(need), clear=names(clear), clear_new=names(clear_new), prior=bool(prior), history=bool(history), m2=bool(m2),
                    motion=bool(motion), color=color, tonemap=tonemap, steps=steps)

    def free(self, event, arg=0):
        gone = names(self.event(event, arg))
        self.planes -= gone
        return gone

    def swap(self, event, arg=0):
        swapped = names(self.event(event, arg))
        twin = {"temporal": "hist", "guide": "hguide", "albedo": "halbedo", "variance": "vhist", "inst": "hinst"}
        assert swapped <= set(twin)
        for a in swapped:
            have_a, have_b = a in self.planes, twin[a] in self.planes
            self.planes -= {a, twin[a]}
            self.planes |= ({twin[a]} if have_a else set()) | ({a} if have_b else set())
        return swapped

    def read_gbuffer(self):
        want_inst = self.features & MOTION and self.features & TEMPORAL
        if not self.flags() & GBUFFER or (want_inst and "inst" not in self.planes):
            self.planes |= {"guide", "albedo"} | ({"inst"} if want_inst else set())
            self.event(GBUFFER_COMPUTED)

    def sync(self):
        assert self.features & (DENOISE | TEMPORAL | VARIANCE)
        p = self.plan()
        self.read_gbuffer()
        self.planes |= p["need"]
        if p["prior"]:
            if p["motion"]:
                self.planes.add("motion_table")
            self.event(PRIOR_COMPUTED)
        self.event(SYNCED)
        return p

    def aovs(self):
        """Per AOV: True (readable) or the refusal's words."""
        out = {}
        for which, name in enumerate(AOV_NAMES):
            why = self.lib.frame_sync_aov_refusal(self.s, C.c_int64(which), C.c_int64(1 if self.features & TEMPORAL else 0),
                                                  C.c_int64(1 if "prior2" in self.planes else 0))
            out[name] = True if why is None else why.decode()
        return out


@pytest.fixture
def state(lib):
    s = State(lib)
    yield s
    s.close()


def new_tracer(s, table=OPTION_OFF):
    """What conftest.make_hip_tracer does to the state: frame size, scene, camera."""
    assert s.free(RESIZED) == set(PLANES)
    assert s.swap(SCENE_CHANGED, table) == set()
    assert s.swap(CAMERA_MOVED) == set()


# ---- (a) the plan of a sync, for every combination of features, history and first / later sync

# by (denoise, temporal, variance): the timed steps, what the filter reads, what the tone-map reads
STEPS = {
    (0, 0, 0): (["tonemap"], ACCUMULATOR, ACCUMULATOR),                                       # (the plain sync: one tone-map of the accumulator)
    (1, 0, 0): (["denoise", "tonemap"], ACCUMULATOR, DENOISED_PLANE),
    (0, 0, 1): (["variance", "tonemap"], ACCUMULATOR, ACCUMULATOR),
    (1, 0, 1): (["variance", "denoise_variance", "tonemap"], ACCUMULATOR, DENOISED_PLANE),
    (0, 1, 0): (["temporal", "tonemap"], TEMPORAL_PLANE, TEMPORAL_PLANE),
    (1, 1, 0): (["temporal", "denoise", "tonemap"], TEMPORAL_PLANE, DENOISED_PLANE),
    (0, 1, 1): (["temporal", "variance", "tonemap"], TEMPORAL_PLANE, TEMPORAL_PLANE),
    (1, 1, 1): (["temporal", "variance", "denoise_variance", "tonemap"], TEMPORAL_PLANE, DENOISED_PLANE),
}
# the planes a feature needs beside the G-buffer's GUIDE and ALBEDO, which every filtered sync needs
NEEDS = {DENOISE: {"denoised", "ping", "pong"}, TEMPORAL: {"temporal", "prior"}, VARIANCE: {"variance"}}


@pytest.mark.parametrize("history", ["none", "without M2", "with M2"])
@pytest.mark.parametrize("later", [False, True])
@pytest.mark.parametrize("d, t, v, m", list(itertools.product((0, 1), repeat=4)))
def test_plan_of_every_feature_combination(state, history, later, d, t, v, m):
    """All 16 combinations of denoise, temporal reuse, variance guidance and object motion; with no history, a history without M2 and
    one with M2; at the first sync under a camera and at a later one."""
    s = state
    new_tracer(s, TABLE)
    if history != "none":   # a temporal sync (with variance guidance: it writes VARIANCE too), then a camera move that captures it
        s.features = TEMPORAL | MOTION | (VARIANCE if history == "with M2" else 0)
        s.sync()
        assert s.swap(CAMERA_MOVED) == {"temporal", "guide", "albedo", "inst"} | ({"variance"} if history == "with M2" else set())
        assert s.flags() == HAVE_HISTORY | (HISTORY_M2 if history == "with M2" else 0)
    f = s.features = d * DENOISE | t * TEMPORAL | v * VARIANCE | m * MOTION
    if later and f & ~MOTION:        # a sync under this camera has run: G-buffer, PRIOR, then the sync's own mark
        s.sync()
    p = s.plan(f)
    steps, color, tonemap = STEPS[d, t, v]
    assert (p["steps"], p["color"], p["tonemap"]) == (steps, color, tonemap), (d, t, v, m)
    need = {"guide", "albedo"} | (NEEDS[DENOISE] if d else set()) | (NEEDS[TEMPORAL] if t else set()) | (NEEDS[VARIANCE] if v else set())
    if t and v:
        need |= {"prior2"}
    if t and m:
        need |= {"inst"}                          # object motion has an effect only with temporal reuse on
    assert p["need"] == need, (d, t, v, m)
    # cleared: TEMPORAL (and with variance guidance VARIANCE) at the first temporal sync under a camera; without temporal reuse
    # VARIANCE when the sync allocates it
    first = t and not later
    assert p["clear"] == (({"temporal"} | ({"variance"} if v else set())) if first else set()), (d, t, v, m)
    assert p["clear_new"] == ({"variance"} if v and not t else set()), (d, t, v, m)
    # PRIOR: stale at the first temporal sync under a camera; kReproject[m2][motion] with a history, cleared without
    assert p["prior"] == bool(first), (d, t, v, m)
    assert p["history"] == bool(first and history != "none"), (d, t, v, m)
    assert p["m2"] == bool(first and v and history == "with M2"), (d, t, v, m)
    assert p["motion"] == bool(first and m and history != "none"), (d, t, v, m)


def test_plane_sets(lib):
    """Every plane is freed with exactly one feature; the moment and motion planes are part of temporal reuse's."""
    denoise, temporal, variance, moment, motion = (names(lib.frame_sync_plane_sets(C.c_int64(i))) for i in range(5))
    assert denoise == {"guide", "albedo", "denoised", "ping", "pong"}
    assert variance == {"variance"}
    assert moment == {"vhist", "prior2"} and motion == {"inst", "hinst", "motion_table"}
    assert temporal == {"temporal", "prior", "hist", "hguide", "halbedo"} | moment | motion
    assert denoise | temporal | variance == set(PLANES) and not (denoise & temporal or denoise & variance or temporal & variance)


# ---- (b) event sequences

def test_replay_of_the_gpu_toggle_and_resize_test(state):
    """The 13 steps of tests/test_gpu_plane_lifetimes.py::test_planes_follow_toggles_and_resizes on the state alone: after every sync
    exactly the AOVs that test reads are readable, the others are refused in the words it compares, and the planes that exist are
    those of the features in force."""
    s = state
    new_tracer(s)
    gbuffer = {"guide", "albedo"}
    filter_planes = {"denoised", "ping", "pong"}

    def check(readable, refusals, planes):
        s.read_gbuffer()                              # (the GPU test's snapshot reads GUIDE first)
        got = s.aovs()
        assert {n for n, r in got.items() if r is True} == readable
        assert {n: r for n, r in got.items() if r is not True} == refusals
        assert s.planes == planes

    s.features = DENOISE                                                            # 1. denoise on
    s.sync()
    check(gbuffer | {"denoised"}, {"temporal": NO_TEMPORAL, "prior": NO_TEMPORAL, "variance": NO_VARIANCE_RESIZE, "prior2": NO_PRIOR2},
          gbuffer | filter_planes)
    s.features |= VARIANCE                                                          # 2. variance on
    assert s.free(VARIANCE_TOGGLED, 1) == set()
    assert s.sync()["clear_new"] == {"variance"}
    check(gbuffer | {"denoised", "variance"}, {"temporal": NO_TEMPORAL, "prior": NO_TEMPORAL, "prior2": NO_PRIOR2}, gbuffer | filter_planes | {"variance"})
    s.features &= ~VARIANCE                                                         # 3. variance off
    assert s.free(VARIANCE_TOGGLED, 0) == {"variance", "vhist", "prior2"}
    assert s.planes == gbuffer | filter_planes
    assert s.free(RESIZED) == set(PLANES) and s.planes == set()                     # 4. the second frame
    assert s.aovs()["denoised"] == NO_DENOISED
    s.features |= VARIANCE                                                          # 5. variance on
    s.free(VARIANCE_TOGGLED, 1)
    s.features |= TEMPORAL                                                          # 6. temporal reuse on
    s.event(TEMPORAL_PARAMS_CHANGED)
    p = s.sync()                                                                    # 7.
    assert p["clear"] == {"temporal", "variance"} and p["prior"] and not p["history"]
    everything = gbuffer | filter_planes | {"temporal", "prior", "variance", "prior2"}
    check(set(AOV_NAMES), {}, everything)
    assert s.swap(CAMERA_MOVED) == {"temporal", "guide", "albedo", "variance"}      # 8. move the camera
    assert s.planes == filter_planes | {"prior", "prior2", "hist", "hguide", "halbedo", "vhist"}
    assert s.aovs()["variance"] == NO_VARIANCE_CAMERA and s.aovs()["temporal"] == NO_TEMPORAL and s.aovs()["prior2"] == NO_PRIOR2
    p = s.sync()                                                                    # 9.
    assert p["clear"] == {"temporal", "variance"} and p["prior"] and p["history"] and p["m2"] and not p["motion"]
    check(set(AOV_NAMES), {}, everything | {"hist", "hguide", "halbedo", "vhist"})
    s.features &= ~TEMPORAL                                                         # 10. temporal reuse off
    assert s.free(TEMPORAL_OFF) == {"temporal", "prior", "hist", "hguide", "halbedo", "vhist", "prior2", "inst", "hinst", "motion_table"}
    s.sync()                                                                        # 11.
    check(gbuffer | {"denoised", "variance"}, {"temporal": NO_TEMPORAL, "prior": NO_TEMPORAL, "prior2": NO_PRIOR2}, gbuffer | filter_planes | {"variance"})
    s.free(RESIZED)                                                                 # 12. back to the first frame
    assert s.planes == set()
    assert s.sync()["clear_new"] == {"variance"}                                    # 13.
    check(gbuffer | {"denoised", "variance"}, {"temporal": NO_TEMPORAL, "prior": NO_TEMPORAL, "prior2": NO_PRIOR2}, gbuffer | filter_planes | {"variance"})


def test_camera_move_without_a_sync_keeps_the_older_history(state):
    s = state
    new_tracer(s)
    s.features = TEMPORAL
    s.sync()
    assert s.swap(CAMERA_MOVED) == {"temporal", "guide", "albedo"}
    assert s.flags() == HAVE_HISTORY and s.planes == {"prior", "hist", "hguide", "halbedo"}
    assert s.swap(CAMERA_MOVED) == set()          # no sync under the second camera: nothing joins the history, which stays
    assert s.flags() == HAVE_HISTORY and s.planes == {"prior", "hist", "hguide", "halbedo"}
    p = s.sync()
    assert p["prior"] and p["history"] and p["clear"] == {"temporal"}
    assert s.flags() == GBUFFER | PRIOR | HAVE_HISTORY | TEMPORAL_SYNCED
    s.features = 0                                # without temporal reuse a camera move only makes the G-buffer stale
    s.event(TEMPORAL_OFF)
    s.event(GBUFFER_COMPUTED)
    assert s.swap(CAMERA_MOVED) == set() and s.flags() == 0


@pytest.mark.parametrize("next_table, kept", [(MOVED, True), (OTHER_MESH, False), (READ_BACK, False), (NO_TABLE, False)])
def test_scene_change_with_object_motion(state, next_table, kept):
    """With object motion a scene change captures the planes synced under the old scene like a camera move; the history survives only
    into a scene with the same instances of the same meshes.  An in-place vertex update passes no table: the history goes, uncaptured."""
    s = state
    new_tracer(s, TABLE)
    s.features = TEMPORAL | VARIANCE | MOTION
    s.sync()
    assert s.planes >= {"inst", "variance", "temporal"}
    swapped = s.swap(SCENE_CHANGED, next_table)
    assert swapped == (set() if next_table == NO_TABLE else {"temporal", "guide", "albedo", "variance", "inst"})
    assert s.flags() == ((HAVE_HISTORY | HISTORY_M2) if kept else 0)      # G-buffer stale, nothing synced, PRIOR stale
    assert s.tables() == (TABLE if next_table == NO_TABLE else next_table, TABLE if next_table != NO_TABLE else OPTION_OFF)
    p = s.sync()
    assert p["prior"] and (p["history"], p["m2"], p["motion"]) == (kept, kept, kept)
    assert ("motion_table" in s.planes) == kept


def test_scene_change_without_object_motion_drops_the_history(state):
    s = state
    new_tracer(s)
    s.features = TEMPORAL
    s.sync()
    s.swap(CAMERA_MOVED)
    s.sync()
    assert s.flags() == GBUFFER | PRIOR | HAVE_HISTORY | TEMPORAL_SYNCED
    assert s.swap(SCENE_CHANGED, OPTION_OFF) == set() and s.flags() == 0
    s.features = DENOISE                       # temporal reuse off: only the G-buffer is the scene's
    s.event(TEMPORAL_OFF)
    s.sync()
    assert s.aovs()["denoised"] is True
    assert s.swap(SCENE_CHANGED, OPTION_OFF) == set() and s.flags() == 0 and s.aovs()["denoised"] is True


def test_temporal_parameter_change_makes_prior_stale(state):
    s = state
    new_tracer(s)
    s.features = TEMPORAL
    s.sync()
    s.swap(CAMERA_MOVED)
    s.sync()
    s.event(TEMPORAL_PARAMS_CHANGED)
    assert s.flags() == GBUFFER | HAVE_HISTORY | TEMPORAL_SYNCED                  # TEMPORAL is kept: not cleared at the next sync
    assert s.aovs()["temporal"] == NO_TEMPORAL and s.aovs()["prior"] == NO_TEMPORAL
    p = s.sync()
    assert p["prior"] and p["history"] and p["clear"] == set()
    assert s.aovs()["temporal"] is True and s.aovs()["prior"] is True


def test_variance_toggled_under_temporal_reuse(state):
    s = state
    new_tracer(s)
    s.features = TEMPORAL
    s.sync()
    s.features |= VARIANCE
    assert s.free(VARIANCE_TOGGLED, 1) == set()
    assert s.flags() == GBUFFER | TEMPORAL_SYNCED                                  # PRIOR stale: the next reprojection writes PRIOR2
    p = s.sync()
    assert p["prior"] and p["clear"] == {"variance"} and p["need"] >= {"variance", "prior2"}
    assert s.flags() == GBUFFER | PRIOR | TEMPORAL_SYNCED | VARIANCE_SYNCED and s.aovs()["prior2"] is True
    assert s.swap(CAMERA_MOVED) == {"temporal", "guide", "albedo", "variance"} and s.flags() == HAVE_HISTORY | HISTORY_M2
    s.sync()
    s.features &= ~VARIANCE
    assert s.free(VARIANCE_TOGGLED, 0) == {"variance", "vhist", "prior2"}
    assert s.flags() == GBUFFER | HAVE_HISTORY | TEMPORAL_SYNCED                   # PRIOR stale again, the history's M2 gone with its plane
    assert s.aovs()["variance"] == NO_VARIANCE_CAMERA and s.aovs()["prior2"] == NO_PRIOR2
    p = s.sync()
    assert p["prior"] and p["history"] and not p["m2"] and p["clear"] == set()


def test_temporal_turned_on_after_a_variance_sync(state):
    """A variance sync without temporal reuse says nothing about a camera: the first temporal sync clears VARIANCE like TEMPORAL, and
    PRIOR2 cannot be read before it."""
    s = state
    new_tracer(s)
    s.features = VARIANCE
    s.free(VARIANCE_TOGGLED, 1)
    s.sync()
    assert s.flags() == GBUFFER and s.aovs()["variance"] is True
    s.features |= TEMPORAL
    s.event(TEMPORAL_PARAMS_CHANGED)
    assert s.aovs()["variance"] is True and s.aovs()["prior2"] == NO_PRIOR2       # (VARIANCE still holds the last sync's rows)
    assert s.sync()["clear"] == {"temporal", "variance"}
    assert s.flags() == GBUFFER | PRIOR | TEMPORAL_SYNCED | VARIANCE_SYNCED and s.aovs()["prior2"] is True


def test_object_motion_toggled(state):
    """Either way the history and the G-buffer go with the old setting and both instance tables are forgotten; DENOISED stays.  Turned
    off, the INSTANCE planes and the motion table go."""
    s = state
    new_tracer(s, TABLE)
    s.features = DENOISE | TEMPORAL | VARIANCE | MOTION
    s.sync()
    s.swap(SCENE_CHANGED, MOVED)
    assert s.sync()["motion"] and s.planes >= {"inst", "hinst", "motion_table"}
    assert s.flags() == GBUFFER | PRIOR | HAVE_HISTORY | HISTORY_M2 | TEMPORAL_SYNCED | VARIANCE_SYNCED and s.tables() == (MOVED, TABLE)
    s.features &= ~MOTION
    assert s.free(MOTION_TOGGLED, 0) == {"inst", "hinst", "motion_table"}
    assert s.flags() == 0 and s.tables() == (OPTION_OFF, OPTION_OFF)
    got = s.aovs()
    assert got["denoised"] is True and got["temporal"] == NO_TEMPORAL and got["variance"] == NO_VARIANCE_CAMERA and got["prior2"] == NO_PRIOR2
    p = s.sync()
    assert p["prior"] and not p["history"] and not p["motion"] and "inst" not in p["need"] and p["clear"] == {"temporal", "variance"}
    s.features |= MOTION
    assert s.free(MOTION_TOGGLED, 1) == set() and s.flags() == 0
    s.lib.frame_sync_set_current_table(s.s, C.c_int64(READ_BACK))                 # (the matrices come back from the device)
    p = s.sync()
    assert p["prior"] and not p["history"] and "inst" in p["need"] and "inst" in s.planes
    assert s.swap(CAMERA_MOVED) == {"temporal", "guide", "albedo", "variance", "inst"} and s.tables() == (READ_BACK, READ_BACK)
    assert s.sync()["motion"]                                                      # camera moves reuse the history at once ...
    assert s.swap(SCENE_CHANGED, TABLE) >= {"inst"} and s.flags() == 0             # ... the first upload after it drops the history
