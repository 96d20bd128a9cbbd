"""CPU tests of editing materials in place (polaris_hip_update_materials; polaris_amd/csrc/material_update.h).

tests/tools/material_update_check.cpp applies the HOST RESTATEMENT of the update -- the argument checks, the classes of the new node
table, the retag of every triangle record (the very function k_retag is made of), the mask of emitting classes -- to
build_layout(base).  The bar, for every case of tests/material_update_cases.py and max_leaf_tris 0, 2 and 4: the triangle records
(every byte), tri_bits and emit_classes equal build_layout(substituted)'s; every OTHER array of the two layouts is byte-equal with no
update applied at all, because nothing but those depends on materials.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import material_update_cases as cases
from conftest import ROOT
from polaris_amd import ctypes_api as T
from polaris_amd import scenes

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "material_update_check.cpp")
LIB = os.path.join(BUILD, "libmaterial_update_check.so")
CAP = 1 << 22
E_BAD_ARGUMENT, E_NO_SCENE_DATA, E_BAD_SCENE = 2, 1, 5
CSRC = os.path.join(ROOT, "polaris_amd", "csrc")
DEPS = [SRC, os.path.join(ROOT, "include", "polaris_hip.h"), os.path.join(CSRC, "scene_layout.h"), os.path.join(CSRC, "material_update.h")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


@pytest.fixture(scope="module")
def tool():
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *INCLUDES, SRC, "-o", LIB])
    return C.CDLL(LIB)


class Out:
    def __init__(self):
        self.tris, self.rest = np.zeros(CAP, np.uint8), np.zeros(CAP, np.uint8)
        self.counts, self.shading = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        self.err = C.create_string_buffer(512)

    def args(self):
        return [C.c_void_p(self.tris.ctypes.data), C.c_void_p(self.rest.ctypes.data), C.c_size_t(CAP), C.c_void_p(self.counts.ctypes.data),
                C.c_void_p(self.shading.ctypes.data)]

    def take(self):
        """(triangle records, the rest of the layout as bytes, tri_bits, emit_classes)"""
        return (self.tris[:int(self.counts[0]) * 48].view(T.TRI_RECORD).copy(), self.rest[:int(self.counts[1])].tobytes(),
                int(self.shading[0]), int(self.shading[1]))


def layout(tool, sc, max_leaf):
    o, view = Out(), T.scene_view(sc)
    rc = tool.mu_layout(C.byref(view), max_leaf, *o.args(), o.err, C.c_size_t(512))
    assert rc == 0, o.err.value.decode()
    return o.take()


def update(tool, base, max_leaf, u, force_tri_bits=0):
    """(layout after the restated update, status, message)"""
    o, view, status = Out(), T.scene_view(base), C.c_int(0)
    rc = tool.mu_update(C.byref(view), max_leaf, C.byref(u) if u is not None else None, force_tri_bits, *o.args(), C.byref(status), o.err, C.c_size_t(512))
    assert rc == 0, o.err.value.decode()
    return o.take(), status.value, o.err.value.decode()


def struct_of(args):
    return T.material_update(args["nodes"], args["material_index"], args["scene_diffuse"], args["emissive_mat_nodes"])


# ---- 1. the restated update against a full layout of the substituted scene -------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [0, 2, 4])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_restated_update_equals_layout_of_substituted_scene(tool, name, max_leaf):
    base, sub, args = cases.case(name)
    want, before = layout(tool, sub, max_leaf), layout(tool, base, max_leaf)
    assert before[1] == want[1], "an array that no update touches depends on materials"
    u, keep = struct_of(args)
    got, status, msg = update(tool, base, max_leaf, u)
    assert status == 0, msg
    assert got[0].tobytes() == want[0].tobytes(), "triangle records"
    assert got[2:] == want[2:] and got[2] == 24, "tri_bits, emit_classes"
    assert got[1] == before[1]
    v0 = lambda t: (t["v0"].tobytes(), t["rank"].tobytes(), t["e1"].tobytes(), t["e2"].tobytes())  # noqa: E731
    assert v0(got[0]) == v0(before[0]), "the retag wrote more than the two words"
    if name in cases.MASK_CHANGES:
        assert got[3] != before[3]
    else:
        assert got[3] == before[3]
    if name in ("recolour", "background"):
        assert got[0].tobytes() == before[0].tobytes()
    elif name not in ("light-off", "class-15"):    # (those two move reach sets inside their class: only the mask changes, which is what they are for)
        assert got[0].tobytes() != before[0].tobytes(), "the case changes no class"
    if name == "new-emitter":
        assert bin(got[3]).count("1") == bin(before[3]).count("1") + 1
    if name == "light-off":
        assert got[3] == 0 and before[3] != 0
    if name == "class-15":
        assert got[3] == before[3] | 1 << 15 and not before[3] >> 15 & 1
        assert (got[0]["orig"] >> 24 == 15).sum() > 12          # more than one material tree shares the class
    if name == "not-tiny":
        assert len(got[0]) > 2046 and not got[0]["word"].any()
    else:
        assert len(got[0]) <= 2046 and got[0]["word"].any()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_without_classes_the_restatement_changes_no_byte(tool, name):
    base, _, args = cases.case(name)
    before = layout(tool, base, 2)
    u, keep = struct_of(args)
    got, status, msg = update(tool, base, 2, u, force_tri_bits=31)
    assert status == 0, msg
    assert got[0].tobytes() == before[0].tobytes() and got[1] == before[1]
    assert got[3] == 0xFFFF


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def _refusals():
    """(what, status, text, args of the update, fields to overwrite in the struct) of every refusal of update_materials."""
    base, _, _ = cases.case("textured")
    nodes = base.material_nodes
    NN, NT = len(nodes), base.num_triangles
    ok = dict(nodes=nodes.copy(), material_index=base.material_index.copy(), scene_diffuse=int(base.scene_diffuse_mat_index),
              emissive_mat_nodes=base.emissives["mat_node_index"].copy(), textures=None)
    mix = int(np.nonzero(nodes["type"] == T.OP_MIX_MAP)[0][0])
    bump = int(np.nonzero(nodes["type"] == T.OP_BUMP_MAP)[0][0])
    disp = int(np.nonzero(nodes["type"] == T.OP_DISPERSE)[0][0])
    diel = int(np.nonzero(nodes["type"] == T.BXDF_ROUGH_DIELECTRIC)[0][0])
    diff = int(np.nonzero(nodes["type"] == T.BXDF_DIFFUSE)[0][0])

    def table(i, field, value):
        n = nodes.copy()
        n[field][i] = value
        return dict(ok, nodes=n)

    def other(key, i, value):
        a = ok[key].copy()
        a[i] = value
        return dict(ok, **{key: a})

    yield "unknown operator", E_BAD_SCENE, f"material node {bump}: unknown operator", table(bump, "type", 10009), {}
    yield "left child", E_BAD_SCENE, f"material node {bump}: left child out of range", table(bump, "left_child", NN), {}
    yield "right child", E_BAD_SCENE, f"material node {mix}: right child out of range", table(mix, "right_child", -1), {}
    yield "operator texture", E_BAD_SCENE, f"material node {bump}: operator texture out of range", table(bump, "tex", -1), {}
    yield "disperse texture", E_BAD_SCENE, f"material node {disp}: texture out of range", table(disp, "tex", len(base.texture_meta)), {}
    yield "leaf texture", E_BAD_SCENE, f"material node {diff}: texture out of range", table(diff, "tex", -2), {}
    yield "roughness texture", E_BAD_SCENE, f"material node {diel}: texture out of range", table(diel, "roughness_tex", 99), {}
    yield "transmittance texture", E_BAD_SCENE, f"material node {diel}: transmittance texture out of range", table(diel, "right_child", 99), {}
    yield "triangle root", E_BAD_SCENE, "triangle 7: material root out of range", other("material_index", 7, NN), {}
    yield "emissive node", E_BAD_SCENE, "emissive 1: material node out of range", other("emissive_mat_nodes", 1, NN + 3), {}
    yield "background", E_BAD_SCENE, "scene diffuse material index out of range", dict(ok, scene_diffuse=NN), {}
    yield "background below -1", E_BAD_SCENE, "scene diffuse material index out of range", dict(ok, scene_diffuse=-2), {}
    yield "struct_size", E_BAD_ARGUMENT, "struct_size", ok, {"struct_size": C.sizeof(T.MaterialUpdate) + 8}
    yield "null nodes", E_BAD_ARGUMENT, "pointer is null", ok, {"material_nodes": None}
    yield "node count", E_BAD_ARGUMENT, "material nodes, the uploaded scene has", dict(ok, nodes=nodes[:-1].copy()), {}
    yield "triangle count", E_BAD_ARGUMENT, "triangles, the uploaded scene has", dict(ok, material_index=base.material_index[:-1].copy()), {}
    yield "emissive count", E_BAD_ARGUMENT, "emissives, the uploaded scene has", dict(ok, emissive_mat_nodes=ok["emissive_mat_nodes"][:-1].copy()), {}


def refusal_struct(args, fields):
    u, keep = struct_of(args)
    for k, v in fields.items():
        setattr(u, k, v)
    return u, keep


def test_refusals_return_their_status_and_the_uploads_text_and_change_nothing(tool):
    base, _, _ = cases.case("textured")
    untouched = layout(tool, base, 2)
    rules = set()
    for what, status, text, args, fields in _refusals():
        u, keep = refusal_struct(args, fields)
        got, st, msg = update(tool, base, 2, u)
        assert st == status and text in msg, (what, st, msg)
        assert got[0].tobytes() == untouched[0].tobytes() and got[1:] == untouched[1:], what
        if status == E_BAD_SCENE:    # the upload's own verdict on the substituted arrays, word for word
            assert msg == text
            sub = scenes.with_materials(base, nodes=args["nodes"], material_index=args["material_index"], scene_diffuse=args["scene_diffuse"],
                                        emissive_mat_nodes=args["emissive_mat_nodes"])
            err, view = C.create_string_buffer(512), T.scene_view(sub)
            assert tool.mu_layout_error(C.byref(view), err, C.c_size_t(512)) == 1 and err.value.decode() == msg, what
            rules.add(msg.split(": ")[-1])
    assert len(rules) == 9       # every material rule of build_layout
    assert update(tool, base, 2, None)[1] == E_BAD_ARGUMENT
    good, keep = struct_of(cases.case("textured")[2])
    assert update(tool, base, 2, good)[1] == 0


def test_texture_refusals(tool):
    base, _, args = cases.case("textured")
    meta = np.ascontiguousarray(base.texture_meta)
    err = C.create_string_buffer(512)

    def check(index, texels, n_bytes=None, have_scene=1):
        t = np.ascontiguousarray(texels)
        rc = tool.mu_texture_check(C.c_void_p(meta.ctypes.data), len(meta), have_scene, index, C.c_void_p(t.ctypes.data), C.c_size_t(t.nbytes if n_bytes is None else n_bytes), err,
                                   C.c_size_t(512))
        return rc, err.value.decode()

    for index, texels in args["textures"].items():
        assert check(index, texels) == (0, "")
        assert check(index, texels, have_scene=0) == (E_NO_SCENE_DATA, "no scene data uploaded")
        rc, msg = check(index, texels, n_bytes=np.ascontiguousarray(texels).nbytes - 4)
        assert rc == E_BAD_ARGUMENT and f"texture {index} has" in msg
    rc, msg = check(len(meta), np.zeros(4, np.uint8))
    assert rc == E_BAD_ARGUMENT and "out of range" in msg
    sizes = {int(m["format"]): int(m["width"]) * int(m["height"]) for m in meta}
    assert set(sizes) == {T.TEX_L8, T.TEX_L32F, T.TEX_RGBA8, T.TEX_RGBA32F}
    for i, m in enumerate(meta):      # the size rule is the upload's: 1, 4, 4 and 16 bytes per texel
        bpp = {T.TEX_L8: 1, T.TEX_L32F: 4, T.TEX_RGBA8: 4, T.TEX_RGBA32F: 16}[int(m["format"])]
        n = bpp * int(m["width"]) * int(m["height"])
        assert check(i, np.zeros(n, np.uint8))[0] == 0 and check(i, np.zeros(n + 1, np.uint8))[0] == E_BAD_ARGUMENT


# ---- 3. the same under the sanitizers, in a program of its own ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan_program():
    out = os.path.join(BUILD, "material_update_check_asan")
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DMU_MAIN",
                               *INCLUDES, SRC, "-o", out])
    return out


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_is_clean_under_asan_and_ubsan(asan_program, name, tmp_path):
    base, _, args = cases.case(name)
    raw = str(tmp_path / "case.bin")
    arrs = [base.bvh_nodes, base.mesh_instances, base.material_nodes, base.emissives, base.texture_meta, base.texture_data, base.vertices, base.normals, base.uvs,
            base.material_index]
    mi, em = args["material_index"], args["emissive_mat_nodes"]
    hdr = np.array([len(a) for a in arrs] + [base.scene_diffuse_mat_index, base.scene_emissive_mat_index, mi is not None, em is not None, args["scene_diffuse"]], dtype=np.int64)
    with open(raw, "wb") as f:
        f.write(hdr.tobytes())
        for a in arrs:
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(np.ascontiguousarray(args["nodes"], dtype=T.MATERIAL_NODE).tobytes())
        if mi is not None:
            f.write(np.ascontiguousarray(mi, dtype=np.uint32).tobytes())
        if em is not None:
            f.write(np.ascontiguousarray(em, dtype=np.uint32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([asan_program, raw], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout[-500:], p.stderr[-3000:])
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]


def test_ctypes_mirror_matches_the_header():
    assert C.sizeof(T.MaterialUpdate) == 56 and T.MaterialUpdate().struct_size == 56
    assert "polaris_hip_update_materials" in T.C_ABI_SYMBOLS and "polaris_hip_update_texture" in T.C_ABI_SYMBOLS
    assert (T.REC_TRIS, T.REC_SHADING) == (3, 4)


def test_recolour_argument_of_the_example_driver():
    from polaris_amd import render

    node, rgb, step = render.parse_recolour("3:0.5,0.25,1:0.1", 13)
    assert node == 3 and rgb.tolist() == [0.5, 0.25, 1.0] and step == np.float32(0.1)
    assert render.parse_recolour("0:1,1,1", 1)[2] == 0
    for bad in ("13:1,1,1", "x:1,1,1", "2:1,1", "2", "2:1,1,1:0.1:7", "-1:1,1,1"):
        with pytest.raises(ValueError):
            render.parse_recolour(bad, 13)


def test_with_materials_shares_geometry_and_material_update_args_round_trip():
    base, sub, args = cases.case("textured")
    for f in ("bvh_nodes", "mesh_instances", "vertices", "normals", "uvs", "texture_meta"):
        assert getattr(sub, f) is getattr(base, f), f
    nodes, mi, bg, em = scenes.material_update_args(sub)
    again = scenes.with_materials(base, nodes, mi, bg, em, args["textures"])
    for f in ("material_nodes", "material_index", "emissives", "texture_data"):
        assert getattr(again, f).tobytes() == getattr(sub, f).tobytes(), f
    assert again.scene_diffuse_mat_index == sub.scene_diffuse_mat_index and sub.texture_data.tobytes() != base.texture_data.tobytes()
