"""CPU test of the transition polaris_hip_set_projection adds to the camera's state machine (polaris_amd/csrc/camera_state.h,
CameraState::set_projection) and of the two refusals it adds to set_lens and set_shutter, against a model written from
include/polaris_hip.h: every refusal, identical bytes and off-and-off do nothing, the todo bits of a change, set_camera keeps the
projection, the lens and the shutter are refused while it is on and accepted after it went off.

tests/tools/projection_state_check.cpp is a stand-alone program built with -fsanitize=address,undefined; it reads a script of calls and
prints what each returned and the state it left.

With the projection never set the header must be the one it was: the same program is built a second time against the camera_state.h
of the commit before the projection (PARENT, from `git show`) and random sequences of the three old setters must print the same
lines from both.  Where the repository's history is not at hand (an export without .git) the parent's lines come from
tests/golden/projection_state_parent.txt, which was recorded from that build (the state's bytes as a hash); with the history at hand
both are compared.
"""
import hashlib
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PARENT = "f8c1ccb"          # the commit before polaris_hip_set_projection
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "projection_state_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "projection_state_parent.txt")
DROP_HISTORY, CAMERA_MOVED, SHUTTER_OFF, PROJECTION_CHANGED = 1, 2, 4, 8          # CameraTodo
REFUSED = -1
PINHOLE, LENS, SHUTTER, SHUTTER_LENS, ORTHO, EQUIRECT = range(6)                  # Generator
f32 = np.float32


def compile_tool(exe, include_first, defines=()):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *["-D" + d for d in defines], "-I" + include_first, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", exe])


@pytest.fixture(scope="module")
def tool():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "projection_state_check")
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "camera_state.h"), os.path.join(ROOT, "include", "polaris_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        compile_tool(exe, os.path.join(ROOT, "polaris_amd", "csrc"))
    return exe


def run(exe, script):
    """One line per call: (todo, generator, flags, state bytes, refusal words)."""
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(script)
    got = []
    for ln in lines:
        todo, gen, flags, state, why = ln.split("|", 4)
        got.append((int(todo), int(gen), [int(x) for x in flags.split()], bytes.fromhex(state), why))
    return got


def pack(values):
    return struct.pack("<%df" % len(values), *[float(f32(v)) for v in values])


def camera(eye=(0.5, 0.25, -1.5), frustum=None):
    fr = frustum if frustum is not None else [-1, 1, 1, 0, 1, 1, 1, 0, -1, -1, 1, 0, 1, -1, 1, 0]
    return "C " + (pack(eye) + pack(fr)).hex()


def lens(ten, size=44):
    return "L " + (struct.pack("<I", size) + pack(ten)).hex()


LENS_OFF, LENS_ON = [0.0] * 10, [2.0, 0, 0, 1, 0.05, 0, 0, 0, 0.05, 0]


def shutter(enabled, camera19=None, lens10=None, size=124):
    return "S " + (struct.pack("<II", size, enabled) + pack(camera19 or [0.25] * 19) + pack(lens10 or LENS_ON)).hex()


BASIS = [0.36, 0.48, 0.8, 0.8, -0.6, 0.0, 0.48, 0.64, -0.6]          # orthonormal: axis, right, up (no float is special)


def projection_bytes(kind, basis=BASIS, extents=(1.5, 1.0, 6.0, 3.0), size=60):
    return struct.pack("<II", size, kind) + pack(basis) + pack(extents)


def projection(kind, **kw):
    return "P " + projection_bytes(kind, **kw).hex()


# ---- the model, from include/polaris_hip.h ----------------------------------------------------------------------------------------
def dot3(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def projection_refusal(p, have_camera, lens_on, shutter_on):
    """The reason set_projection refuses these bytes in this state (a word that the refusal's text contains), or None."""
    if p is None or struct.unpack_from("<I", p)[0] != 60:
        return "struct_size"
    kind = struct.unpack_from("<I", p, 4)[0]
    if kind > 2:
        return "kind"
    if kind == 0:
        return None
    if not have_camera:
        return "camera not set"
    fl = [f32(x) for x in struct.unpack_from("<13f", p, 8)]
    if not all(math.isfinite(x) for x in fl):
        return "not finite"
    vec = [fl[0:3], fl[3:6], fl[6:9]]
    for v in vec:
        if not f32(0.998) <= dot3(v, v) <= f32(1.002):
            return "unit vector"
    for k in range(3):
        if not abs(dot3(vec[k], vec[(k + 1) % 3])) <= f32(1e-3):
            return "orthogonal"
    if kind == 1:
        for name, x in (("half_width", fl[9]), ("half_height", fl[10])):
            if not f32(1e-6) <= x <= f32(1e30):
                return name
    else:
        if not f32(1e-3) <= fl[11] <= f32(6.2831855):
            return "lon_range"
        if not f32(1e-3) <= fl[12] <= f32(3.1415927):
            return "lat_range"
    if lens_on:
        return "lens is on"
    if shutter_on:
        return "shutter is on"
    return None


class Model:
    def __init__(self):
        self.have_camera, self.lens_on, self.shutter_on = False, False, False
        self.projection = projection_bytes(0, [0.0] * 9, [0.0] * 4)

    def kind(self):
        return struct.unpack_from("<I", self.projection, 4)[0]

    def set_projection(self, p, commit=True):
        why = projection_refusal(p, self.have_camera, self.lens_on, self.shutter_on)
        if why:
            return REFUSED, why
        kind = struct.unpack_from("<I", p, 4)[0]
        if kind == 0:
            if self.kind() == 0:
                return 0, None                                  # off and off: nothing happens
            if commit:
                self.projection = self.projection[:4] + struct.pack("<I", 0) + self.projection[8:]
            return PROJECTION_CHANGED, None
        if p == self.projection:
            return 0, None                                      # identical bytes: nothing happens
        if commit:
            self.projection = p
        return PROJECTION_CHANGED, None


def check_projection_calls(tool, prefix, calls, model=None):
    """Run prefix (calls of the old setters, which the model is told about by hand) and then the projection calls, each against the model."""
    model = model or Model()
    got = run(tool, prefix + [("P " if commit else "p ") + (p.hex() if p is not None else "null") for p, commit in calls])
    for (p, commit), (todo, gen, flags, state, why) in zip(calls, got[len(prefix):]):
        want_todo, want_why = model.set_projection(p, commit)
        assert todo == want_todo, (p and p.hex(), commit, why, want_why)
        if want_why:
            assert want_why in why, (why, want_why)
        else:
            assert why == ""
        assert state[-60:] == model.projection
        assert flags[2] == int(model.kind() != 0)
        assert gen == (ORTHO if model.kind() == 1 else EQUIRECT) if model.kind() else gen in (PINHOLE, LENS, SHUTTER, SHUTTER_LENS)
    return model, got


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
def bad_projections(kind):
    """(what, bytes) of every refusal of a projection of this kind that does not depend on the state, each one field away from a good one."""
    def but(index, value, k=kind):
        fl = list(BASIS) + [1.5, 1.0, 6.0, 3.0]
        fl[index] = value
        return struct.pack("<II", 60, k) + pack(fl)

    cases = [("struct_size 56", projection_bytes(kind, size=56)), ("struct_size 64", projection_bytes(kind, size=64)), ("struct_size 0", projection_bytes(kind, size=0)),
             ("kind 3", projection_bytes(3)), ("kind 2^31", projection_bytes(1 << 31))]
    for i in range(13):
        for bad in (float("nan"), float("inf"), float("-inf")):
            cases.append((f"float {i} = {bad}", but(i, bad)))
    for v in range(3):
        short, long_ = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        short[v], long_[v] = 0.9985, 1.0015                     # squared 0.9970 and 1.0030
        for name, vec in (("short", short), ("long", long_), ("zero", [0.0, 0.0, 0.0])):
            basis = list(BASIS)
            basis[3 * v:3 * v + 3] = vec
            cases.append((f"{name} vector {v}", projection_bytes(kind, basis)))
    tilt = list(BASIS)
    tilt[3:6] = [0.8 + 0.36 * 2e-3, -0.6 + 0.48 * 2e-3, 0.8 * 2e-3]    # right leans 2e-3 toward the axis
    cases.append(("right leans toward the axis", projection_bytes(kind, tilt)))
    tilt = list(BASIS)
    tilt[6:9] = [0.48 + 0.8 * 2e-3, 0.64 - 0.6 * 2e-3, -0.6]           # up leans 2e-3 toward right
    cases.append(("up leans toward right", projection_bytes(kind, tilt)))
    if kind == 1:
        for i in (9, 10):
            cases += [(f"extent {i} = {x}", but(i, x)) for x in (0.0, -1.0, 0.99e-6, 1.01e30)]
    else:
        cases += [(f"lon_range {x}", but(11, x)) for x in (0.0, -1.0, 0.99e-3, 6.2832, 7.0)]
        cases += [(f"lat_range {x}", but(12, x)) for x in (0.0, -1.0, 0.99e-3, 3.1416, 4.0)]
    return cases


@pytest.mark.parametrize("kind", [1, 2])
def test_every_refusal_changes_nothing(tool, kind):
    good = projection_bytes(kind)
    cases = bad_projections(kind)
    calls = [(None, True), (good, True)]                        # (no camera yet: the good one is refused too)
    model, got = check_projection_calls(tool, [], calls)
    assert [g[0] for g in got] == [REFUSED, REFUSED] and "camera not set" in got[1][4]
    for state_name, first in (("off", None), ("on", good)):
        calls = ([(first, True)] if first else []) + [(None, True)] + [(p, True) for _, p in cases] + [(good, True)]
        model = Model()
        model.have_camera = True
        model, got = check_projection_calls(tool, [camera()], calls, model)
        results = got[1:]
        if first:
            assert results[0][0] == PROJECTION_CHANGED
            results = results[1:]
        for (what, _), g in zip([("null", None)] + cases, results[:-1]):
            assert g[0] == REFUSED and g[4], (state_name, what)
            assert g[3] == results[0][3], (state_name, what)     # every byte of the state as it was
        assert results[-1][0] == (0 if first else PROJECTION_CHANGED), state_name
    # the two fields of the other kind are not range-checked; they must still be finite (above)
    other = list(BASIS) + ([1.5, 1.0, 100.0, -5.0] if kind == 1 else [0.0, -3.0, 6.0, 3.0])
    model = Model()
    model.have_camera = True
    _, got = check_projection_calls(tool, [camera()], [(struct.pack("<II", 60, kind) + pack(other), True)], model)
    assert got[-1][0] == PROJECTION_CHANGED


def test_identical_bytes_off_and_off_and_the_todo_bits(tool):
    ortho, pano = projection_bytes(1), projection_bytes(2)
    garbage_off = struct.pack("<II", 60, 0) + pack([float("nan")] * 13)          # kind 0: nothing else is looked at
    model = Model()
    model.have_camera = True
    calls = [(garbage_off, True), (projection_bytes(0), True),                    # off and off: nothing
             (ortho, False), (ortho, True), (ortho, True),                        # not committed: asked again it is a change again; then identical bytes
             (projection_bytes(1, extents=(1.5, 1.0, 6.0, 3.5)), True),           # a byte of a field the kind does not read: still a change
             (pano, True), (pano, True), (garbage_off, True), (garbage_off, True), (pano, True)]
    _, got = check_projection_calls(tool, [camera()], calls, model)
    assert [g[0] for g in got[1:]] == [0, 0, 8, 8, 0, 8, 8, 0, 8, 0, 8]
    assert [g[1] for g in got[1:]] == [PINHOLE, PINHOLE, PINHOLE, ORTHO, ORTHO, ORTHO, EQUIRECT, EQUIRECT, PINHOLE, PINHOLE, EQUIRECT]


def test_set_camera_keeps_the_projection_and_is_an_ordinary_move(tool):
    pano = projection_bytes(2)
    got = run(tool, [camera(), "P " + pano.hex(), camera(eye=(1.0, 2.0, 3.0)), "P " + pano.hex()])
    assert [g[0] for g in got] == [CAMERA_MOVED, PROJECTION_CHANGED, CAMERA_MOVED, 0]
    assert got[2][1] == EQUIRECT and got[2][2] == [0, 0, 1] and got[2][3][-60:] == pano
    assert got[2][3][4:16] == pack((1.0, 2.0, 3.0))


def test_the_lens_and_the_shutter_are_refused_while_a_projection_is_on(tool):
    ortho = "P " + projection_bytes(1).hex()
    off = "P " + projection_bytes(0).hex()
    got = run(tool, [camera(), ortho,
                     lens(LENS_ON), lens(LENS_OFF), shutter(1), shutter(0),       # on: refused, refused; off: nothing happens, as ever
                     off, lens(LENS_ON), shutter(1),                              # after the projection went off both are accepted
                     ortho, shutter(0), ortho, lens(LENS_OFF), ortho])            # ... and now they refuse the projection, one after the other
    todo = [g[0] for g in got]
    assert todo == [CAMERA_MOVED, PROJECTION_CHANGED, REFUSED, 0, REFUSED, 0, PROJECTION_CHANGED, DROP_HISTORY, DROP_HISTORY,
                    REFUSED, DROP_HISTORY | SHUTTER_OFF, REFUSED, DROP_HISTORY, PROJECTION_CHANGED]
    assert "projection" in got[2][4] and got[2][4].startswith("set_lens") and "projection" in got[4][4] and got[4][4].startswith("set_shutter")
    assert got[2][3] == got[1][3] and got[4][3] == got[1][3]                      # a refusal changes nothing
    assert "lens is on" in got[9][4] and "lens is on" in got[11][4]
    assert [g[1] for g in got[6:9]] == [PINHOLE, LENS, SHUTTER_LENS] and got[13][1] == ORTHO
    # with the lens off and the shutter on, it is the shutter that refuses the projection
    got = run(tool, [camera(), shutter(1), ortho])
    assert got[2][0] == REFUSED and "shutter is on" in got[2][4]


# ---- with the projection never set the header is the parent's ------------------------------------------------------------------------
def old_setter_script(rng, calls=60):
    """A random sequence of the three old setters, refusals among them."""
    script = []
    for _ in range(calls):
        r = rng.random()
        lower = rng.random() < 0.1
        if r < 0.3:
            ln = camera(eye=rng.standard_normal(3), frustum=list(rng.standard_normal(16))) if rng.random() < 0.9 else "C null"
        elif r < 0.65:
            ten = list(LENS_ON) if rng.random() < 0.6 else list(LENS_OFF)
            if rng.random() < 0.5:
                ten[0] = float(rng.choice([0.5, 3.0, 0.0, float("nan"), 2e30]))
            if rng.random() < 0.2:
                ten[int(rng.integers(1, 10))] = float(rng.choice([0.7, float("inf"), 2.0 ** 31]))
            ln = lens(ten, size=44 if rng.random() < 0.9 else 40) if rng.random() < 0.95 else "L null"
        else:
            cam19 = list(rng.standard_normal(19))
            if rng.random() < 0.1:
                cam19[int(rng.integers(0, 19))] = float("nan")
            l10 = list(LENS_ON)
            if rng.random() < 0.3:
                l10[int(rng.integers(0, 10))] = float(rng.choice([0.0, 0.3, float("nan"), 2.0 ** 31]))
            ln = shutter(int(rng.choice([0, 1, 1, 1, 2])), cam19, l10, size=124 if rng.random() < 0.9 else 120) if rng.random() < 0.95 else "S null"
        script.append(ln[0].lower() + ln[1:] if lower else ln)
    return script


def digest(line):
    """A line of the program's output as the golden file keeps it: the state's bytes as a hash (they are 248 bytes a line)."""
    todo, gen, flags, state, why = line.split("|", 4)
    return "|".join((todo, gen, flags, hashlib.sha256(bytes.fromhex(state)).hexdigest()[:16], why))


def without_projection(results):
    return ["%d|%d|%d %d|%s|%s" % (todo, gen, flags[0], flags[1], state[:-60].hex(), why) for todo, gen, flags, state, why in results]


def test_with_the_projection_never_set_every_transition_is_the_parent_commits(tool, tmp_path):
    rng = np.random.default_rng(20261021)
    script = [ln for _ in range(40) for ln in old_setter_script(rng)]
    got = run(tool, script)
    assert all(g[2][2] == 0 and g[3][-60:] == projection_bytes(0, [0.0] * 9, [0.0] * 4) for g in got)
    mine = without_projection(got)
    assert sum(ln.startswith("-1|") for ln in mine) > 100 and len({ln.split("|")[1] for ln in mine}) == 4       # refusals, and all four generators
    with open(GOLDEN) as f:
        recorded = f.read().splitlines()
    assert [digest(ln) for ln in mine] == recorded
    shown = subprocess.run(["git", "-C", ROOT, "show", PARENT + ":polaris_amd/csrc/camera_state.h"], capture_output=True, text=True)
    if shown.returncode == 0:                                   # the repository's history is at hand: the parent's header itself
        (tmp_path / "camera_state.h").write_text(shown.stdout)
        assert "set_projection" not in shown.stdout
        exe = str(tmp_path / "projection_state_check_parent")
        compile_tool(exe, str(tmp_path), defines=["POLARIS_NO_PROJECTION"])
        out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.splitlines() == mine
