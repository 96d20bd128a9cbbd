"""CPU test of the rules that tie polaris_hip_set_camera, polaris_hip_set_lens and polaris_hip_set_shutter together
(polaris_amd/csrc/camera_state.h): random sequences of the three setters against a small model that restates the rules --

  a new camera switches the shutter off; a changed lens switches the shutter off and drops the temporal history; identical bytes do
  nothing; a shutter needs a camera; the close lens is checked only while the lens is on; a refusal changes nothing

-- with the refusals of include/polaris_hip.h in the words the library has always used.  After every call the returned action, the
refusal's words, every byte of the state and the generator it asks for are the model's.  tests/tools/camera_state_check.cpp hands
the caller's bytes to the header; the model below is written from the public header and DESIGN.md 10h / 10j, not from camera_state.h.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "camera_state_check.cpp")
LIB = os.path.join(BUILD, "libcamera_state_check.so")

SET_CAMERA, SET_LENS, SET_SHUTTER = range(3)
DROP_HISTORY, CAMERA_MOVED, SHUTTER_OFF = 1, 2, 4          # what the owner does (CameraTodo)
REFUSED = -1
PINHOLE, LENS, SHUTTER, SHUTTER_LENS = range(4)            # k_generate, k_generate_lens, k_generate_shutter<false>, <true>
LENS_SIZE, SHUTTER_SIZE = 44, 124
SEQUENCES, CALLS = 200, 40

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "camera_state.h"), os.path.join(ROOT, "include", "polaris_hip.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    so.camera_state_new.restype = C.c_void_p
    so.camera_state_delete.restype = None
    for name in ("camera_state_call", "camera_state_bytes", "camera_state_generator"):
        getattr(so, name).restype = C.c_int64
    return so


def floats(b):
    return [f32(x) for x in struct.unpack("<%df" % (len(b) // 4), b)]


def pack(values):
    return struct.pack("<%df" % len(values), *[float(f32(v)) for v in values])


def lens_params(ten, struct_size=LENS_SIZE):
    return struct.pack("<I", struct_size) + pack(ten)


def shutter_params(enabled, camera19, lens10, struct_size=SHUTTER_SIZE):
    return struct.pack("<II", struct_size, enabled) + pack(camera19) + pack(lens10)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def lens_refusal(who, ten, on):
    """set_lens' rules for ten floats (focus distance, axis, u, v): (words, what) or None."""
    for i, x in enumerate(ten):
        if not math.isfinite(x):
            return "%s: float %d is not finite" % (who, i), ("not finite", i)
    if any(abs(x) > f32(2.0 ** 30) for x in ten[4:]):
        return "%s: an entry of u or v is above 2^30" % who, ("above 2^30",)
    if not on:
        return None
    if not f32(1e-6) <= ten[0] <= f32(1e30):
        return "%s: focus_distance %g outside [1e-6, 1e30]" % (who, float(ten[0])), ("focus",)
    a2 = f32(f32(ten[1] * ten[1]) + f32(ten[2] * ten[2])) + f32(ten[3] * ten[3])
    if not f32(0.998) <= a2 <= f32(1.002):
        return "%s: axis is not a unit vector (squared length %g)" % (who, float(a2)), ("axis",)
    return None


class Model:
    """The state as bytes, and per setter: (action or REFUSED, the refusal's words, what happened -- for the coverage count)."""

    def __init__(self):
        self.have_camera = False
        self.camera = pack([0.0] * 19)
        self.lens = lens_params([0.0] * 10)
        self.shutter = shutter_params(0, [0.0] * 19, [0.0] * 10)

    def bytes(self):
        return struct.pack("<I", int(self.have_camera)) + self.camera + self.lens + self.shutter

    def lens_on(self):
        return any(x != 0.0 for x in floats(self.lens[4:])[4:])

    def shutter_on(self):
        return struct.unpack_from("<I", self.shutter, 4)[0] != 0

    def generator(self):
        return (SHUTTER_LENS if self.lens_on() else SHUTTER) if self.shutter_on() else (LENS if self.lens_on() else PINHOLE)

    def shutter_goes_off(self):
        self.shutter = self.shutter[:4] + struct.pack("<I", 0) + self.shutter[8:]

    def set_camera(self, eye, frustum, commit=True):
        if eye is None or frustum is None:
            return REFUSED, "camera pointers are null", ("camera", "null")
        action = CAMERA_MOVED | (SHUTTER_OFF | DROP_HISTORY if self.shutter_on() else 0)      # the close state belonged to the camera that goes
        if commit:
            self.shutter_goes_off()
            self.camera, self.have_camera = eye + frustum, True
        return action, "", ("camera", "set, shutter on" if action & SHUTTER_OFF else "set")

    def set_lens(self, p, commit=True):
        if p is None or struct.unpack_from("<I", p)[0] != LENS_SIZE:
            return REFUSED, "set_lens: null params or struct_size != 44", ("lens", "struct_size")
        ten = floats(p[4:])
        on = any(x != 0.0 for x in ten[4:])
        why = lens_refusal("set_lens", ten, on)
        if why:
            return REFUSED, why[0], ("lens",) + why[1]
        if p == self.lens:
            return 0, "", ("lens", "identical bytes")
        action = DROP_HISTORY | (SHUTTER_OFF if self.shutter_on() else 0)                       # the close lens belonged to the lens that goes
        if commit:
            self.shutter_goes_off()
            self.lens = p
        return action, "", ("lens", "changed, shutter on" if action & SHUTTER_OFF else "changed")

    def set_shutter(self, p, commit=True):
        if p is None or struct.unpack_from("<I", p)[0] != SHUTTER_SIZE:
            return REFUSED, "set_shutter: null params or struct_size != 124", ("shutter", "struct_size")
        enabled = struct.unpack_from("<I", p, 4)[0]
        if enabled > 1:
            return REFUSED, "set_shutter: enabled is %u (0 or 1)" % enabled, ("shutter", "enabled")
        if not self.have_camera:
            return REFUSED, "set_shutter: camera not set (the close state belongs to an open one)", ("shutter", "no camera")
        if enabled:
            for i, x in enumerate(floats(p[8:84])):
                if not math.isfinite(x):
                    return REFUSED, "set_shutter: camera float %d is not finite" % i, ("shutter", "camera float", i)
            if self.lens_on():                                      # the close lens is a lens that is on, whatever its u1 and v1
                why = lens_refusal("set_shutter: close lens", floats(p[84:]), True)
                if why:
                    return REFUSED, why[0], ("close lens",) + why[1]
        if (p == self.shutter) if enabled else not self.shutter_on():
            return 0, "", ("shutter", "identical bytes" if enabled else "off and off")
        if commit:
            if enabled:
                self.shutter = p
            else:
                self.shutter_goes_off()
        return DROP_HISTORY | (0 if enabled else SHUTTER_OFF), "", ("shutter", "on" if enabled else "off")


# ---- the calls of a sequence ---------------------------------------------------------------------------------------------------
NON_FINITE = (float("nan"), float("inf"), float("-inf"))
BAD_FOCUS = (0.0, -1.0, 0.99e-6, 1.01e30)
BAD_AXES = ((0.0, 0.0, 0.9985), (0.0, 0.0, 1.0015), (0.0, 0.0, 0.0))
GOOD_CLOSE_CAMERA = [0.5, 1.0, -2.0] + [(-1.0, 1.0, -1.0, 0.0, 1.0, 1.0, -1.0, 0.0, -1.0, -1.0, -1.0, 0.0, 1.0, -1.0, -1.0, 0.0)[k] for k in range(16)]
# close lenses that set_lens' rules refuse for a lens that is on: each is sent with the lens on (refused) and with it off (accepted)
BAD_CLOSE_LENSES = [[float("nan"), 0, 0, 1, 0.1, 0, 0, 0, 0.1, 0], [2.0, 0, 0, 1, 0.1, 2.0 ** 31, 0, 0, 0.1, 0], [0.0, 0, 0, 1, 0.1, 0, 0, 0, 0.1, 0],
                    [2.0, 0, 0, 0.9985, 0.1, 0, 0, 0, 0.1, 0], [2.0, 0, float("inf"), 1, 0, 0, 0, 0, 0, 0], [1.01e30, 0, 1, 0, 0, 0, 0, 0, 0, 0]]


class Calls:
    """Draws the next call of a sequence.  Which float a refusal spoils cycles through every position, so coverage is by construction."""

    def __init__(self):
        self.turn = 0
        self.last = {SET_LENS: None, SET_SHUTTER: None}

    def good_lens(self, rng, on=True):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        focus = (1e-6, 1e30, 10.0 ** rng.uniform(-5, 29))[min(rng.randint(8), 2)]           # (the edges of the range are accepted)
        uv = rng.uniform(-1, 1, size=6) * 10.0 ** rng.uniform(-3, 8) if on else np.zeros(6)
        if on and rng.randint(8) == 0:
            uv[rng.randint(6)] = (2.0 ** 30, -2.0 ** 30)[rng.randint(2)]                     # (so is 2^30 itself)
        return [focus] + list(axis) + list(uv)

    def good_camera(self, rng):
        return list(rng.uniform(-5, 5, size=19))

    def draw(self, rng):
        self.turn += 1
        t = self.turn
        kind = rng.choice(["camera", "lens", "lens off", "shutter", "shutter off", "repeat", "bad lens", "bad shutter", "bad close lens", "null"],
                          p=[0.12, 0.14, 0.06, 0.16, 0.06, 0.12, 0.12, 0.10, 0.10, 0.02])
        if kind == "camera":
            c = pack(self.good_camera(rng))
            return SET_CAMERA, c[:12], c[12:]
        if kind == "null":
            return [(SET_CAMERA, None, None), (SET_LENS, None, None), (SET_SHUTTER, None, None)][t % 3]
        if kind == "repeat":                                        # the bytes of the last lens or shutter call, whatever became of it
            setter = (SET_LENS, SET_SHUTTER)[t % 2]
            if self.last[setter] is not None:
                return setter, self.last[setter], None
            kind = "lens" if setter == SET_LENS else "shutter"
        if kind in ("lens", "lens off"):
            return self.keep(SET_LENS, lens_params(self.good_lens(rng, on=kind == "lens")))
        if kind == "shutter":                                       # (a close lens with u1 = v1 = 0 is allowed: the aperture closes)
            return self.keep(SET_SHUTTER, shutter_params(1, self.good_camera(rng), self.good_lens(rng, on=rng.randint(4) != 0)))
        if kind == "shutter off":                                   # enabled = 0: nothing else is looked at
            camera = self.good_camera(rng)
            camera[t % 19] = NON_FINITE[t % 3]
            return self.keep(SET_SHUTTER, shutter_params(0, camera, BAD_CLOSE_LENSES[t % len(BAD_CLOSE_LENSES)]))
        if kind == "bad close lens":
            return self.keep(SET_SHUTTER, shutter_params(1, GOOD_CLOSE_CAMERA, BAD_CLOSE_LENSES[t % len(BAD_CLOSE_LENSES)]))
        if kind == "bad lens":
            ten, how = self.good_lens(rng), t % 5
            if how == 0:
                return self.keep(SET_LENS, lens_params(ten, struct_size=(40, 48, 0, 124)[t // 5 % 4]))
            self.spoil(ten, how, t // 5)
            return self.keep(SET_LENS, lens_params(ten))
        camera, ten, how = self.good_camera(rng), self.good_lens(rng), t % 8       # bad shutter
        if how == 0:
            return self.keep(SET_SHUTTER, shutter_params(1, camera, ten, struct_size=(0, 120, 128, 44)[t // 8 % 4]))
        if how == 1:
            return self.keep(SET_SHUTTER, shutter_params((2, 0xFFFFFFFF)[t // 8 % 2], camera, ten))
        if how in (2, 3, 7):
            camera[t // 8 % 19] = NON_FINITE[t // (8 * 19) % 3]
            return self.keep(SET_SHUTTER, shutter_params(1, camera, ten))
        self.spoil(ten, 1 if how in (4, 5) else 2 + t // 8 % 3, t // 8 if how in (4, 5) else t // 24)      # the close lens: refused while the lens is on
        return self.keep(SET_SHUTTER, shutter_params(1, camera, ten))

    @staticmethod
    def spoil(ten, how, n):
        """One field of a good lens that is on, made bad: 1 a non-finite float, 2 u or v above 2^30, 3 the focus distance, 4 the axis."""
        if how == 1:
            ten[n % 10] = NON_FINITE[n // 10 % 3]
        elif how == 2:
            ten[4 + n % 6] = (2.0 ** 30 * 1.001, -2.0 ** 31)[n // 6 % 2]
        elif how == 3:
            ten[0] = BAD_FOCUS[n % 4]
        else:
            ten[1:4] = BAD_AXES[n % 3]

    def keep(self, setter, p):
        self.last[setter] = p
        return setter, p, None


def test_random_setter_sequences_follow_the_model(lib):
    seen, generators, both_ways = set(), set(), {}
    why = C.create_string_buffer(512)
    state = C.create_string_buffer(4 + 19 * 4 + LENS_SIZE + SHUTTER_SIZE)
    calls = Calls()
    for seq in range(SEQUENCES):
        rng = np.random.RandomState(20240 + seq)
        s, m = C.c_void_p(lib.camera_state_new()), Model()
        try:
            for n in range(CALLS):
                setter, a, b = calls.draw(rng)
                commit = rng.randint(10) != 0                      # one call in ten: the owner's own step fails, nothing is committed
                before = m.bytes()
                want_action, want_why, what = (m.set_camera, m.set_lens, m.set_shutter)[setter](*((a, b) if setter == SET_CAMERA else (a,)), commit=commit)
                got_action = lib.camera_state_call(s, C.c_int64(setter), a, b, C.c_int64(commit), why, C.c_int64(len(why)))
                where = (seq, n, what)
                assert got_action == want_action, where
                assert why.value.decode() == want_why, where
                assert lib.camera_state_bytes(s, state) == len(state) and state.raw == m.bytes(), where
                assert lib.camera_state_generator(s) == m.generator() | (4 if m.lens_on() else 0) | (8 if m.shutter_on() else 0), where
                if want_action == REFUSED or want_action == 0 or not commit:
                    assert m.bytes() == before, where                # (the model itself: a refusal changes nothing)
                seen.add(what)
                generators.add(m.generator())
                if setter == SET_SHUTTER and a is not None and a[:8] == struct.pack("<II", SHUTTER_SIZE, 1) and a[8:84] == pack(GOOD_CLOSE_CAMERA) and m.have_camera:
                    both_ways.setdefault(a[84:], set()).add("refused" if want_action == REFUSED else "accepted with the lens off")
        finally:
            lib.camera_state_delete(s)
    # coverage: every refusal tests/test_gpu_lens.py and tests/test_gpu_shutter.py exercise, every outcome, every generator
    want = {("camera", "null"), ("camera", "set"), ("camera", "set, shutter on"),
            ("lens", "struct_size"), ("lens", "above 2^30"), ("lens", "focus"), ("lens", "axis"), ("lens", "identical bytes"), ("lens", "changed"),
            ("lens", "changed, shutter on"),
            ("shutter", "struct_size"), ("shutter", "enabled"), ("shutter", "no camera"), ("shutter", "identical bytes"), ("shutter", "off and off"),
            ("shutter", "on"), ("shutter", "off"),
            ("close lens", "above 2^30"), ("close lens", "focus"), ("close lens", "axis")}
    want |= {("lens", "not finite", i) for i in range(10)} | {("close lens", "not finite", i) for i in range(10)}
    want |= {("shutter", "camera float", i) for i in range(19)}
    assert want <= seen, sorted(want - seen, key=str)
    assert generators == {PINHOLE, LENS, SHUTTER, SHUTTER_LENS}
    assert len(both_ways) == len(BAD_CLOSE_LENSES) and all(v == {"refused", "accepted with the lens off"} for v in both_ways.values()), both_ways


def test_the_order_camera_lens_shutter_and_what_undoes_it(lib):
    """The sequence the layers above re-apply, by hand: camera, lens, shutter give k_generate_shutter<true>; a byte-identical lens
    keeps it; a changed lens or a new camera switches the shutter off; a failed step of the owner's commits nothing."""
    why = C.create_string_buffer(512)
    s = C.c_void_p(lib.camera_state_new())

    def call(setter, a, b=None, commit=1):
        return lib.camera_state_call(s, C.c_int64(setter), a, b, C.c_int64(commit), why, C.c_int64(len(why)))

    try:
        camera = pack(GOOD_CLOSE_CAMERA)
        lens = lens_params([2.0, 0, 0, 1, 0.1, 0, 0, 0, 0.1, 0])
        shutter = shutter_params(1, GOOD_CLOSE_CAMERA, [3.0, 0, 0, 1, 0.1, 0, 0, 0, 0.1, 0])
        assert lib.camera_state_generator(s) == PINHOLE
        assert call(SET_SHUTTER, shutter) == REFUSED and why.value == b"set_shutter: camera not set (the close state belongs to an open one)"
        assert call(SET_CAMERA, camera[:12], camera[12:]) == CAMERA_MOVED
        assert call(SET_LENS, lens, commit=0) == DROP_HISTORY and lib.camera_state_generator(s) == PINHOLE
        assert call(SET_LENS, lens) == DROP_HISTORY and lib.camera_state_generator(s) == LENS | 4
        assert call(SET_SHUTTER, shutter) == DROP_HISTORY and lib.camera_state_generator(s) == SHUTTER_LENS | 4 | 8
        assert call(SET_SHUTTER, shutter) == 0 and call(SET_LENS, lens) == 0 and lib.camera_state_generator(s) == SHUTTER_LENS | 4 | 8
        assert call(SET_LENS, lens_params([2.5, 0, 0, 1, 0.1, 0, 0, 0, 0.1, 0])) == DROP_HISTORY | SHUTTER_OFF and lib.camera_state_generator(s) == LENS | 4
        assert call(SET_SHUTTER, shutter) == DROP_HISTORY
        assert call(SET_CAMERA, camera[:12], camera[12:]) == CAMERA_MOVED | SHUTTER_OFF | DROP_HISTORY and lib.camera_state_generator(s) == LENS | 4
        assert call(SET_SHUTTER, shutter_params(0, [float("nan")] * 19, [float("nan")] * 10)) == 0        # off and off
        assert call(SET_LENS, lens_params([float("-inf"), 9, 9, 9, 0, 0, 0, 0, 0, 0])) == REFUSED and why.value == b"set_lens: float 0 is not finite"
        assert call(SET_LENS, lens_params([-7.0, 9, 9, 9, 0, 0, 0, 0, 0, 0])) == DROP_HISTORY and lib.camera_state_generator(s) == PINHOLE      # off: nothing else is looked at
        assert call(SET_SHUTTER, shutter_params(1, GOOD_CLOSE_CAMERA, BAD_CLOSE_LENSES[2])) == DROP_HISTORY and lib.camera_state_generator(s) == SHUTTER | 8
    finally:
        lib.camera_state_delete(s)
