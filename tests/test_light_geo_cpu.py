"""CPU test of the packed area-light records (polaris_amd/csrc/scene_layout.h: pack_light_geo, derive_light_geo; shading.h, SceneT::light_geo).

upload_scene and update_vertices pack the records with pack_light_geo; tests/tools/light_geo_check.cpp compiles the header alone
(g++, no HIP, -ffp-contract=off as the library).  The bar is a numpy float32 restatement, written operation by operation in the order
derive_light_geo documents -- the multiply-add chain of mul4x1 left to right, the cross product, 1 / sqrt, 1 / area -- so the two
compare BIT FOR BIT: every operation is one IEEE binary32 operation on both sides, and sqrt and division are correctly rounded.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits
from polaris_amd import ctypes_api as T

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "light_geo_check.cpp")
LIB = os.path.join(BUILD, "liblight_geo_check.so")
F = np.float32
GEO = 48   # floats of a record: v0 v1 v2 | n0 n1 n2 (xyz + pad each) | uv0 uv1 uv2, 1 / area, pad | v0', e1', e2', unit normal (xyz + pad each)


@pytest.fixture(scope="module")
def tool():
    os.makedirs(BUILD, exist_ok=True)
    csrc, inc = os.path.join(ROOT, "polaris_amd", "csrc"), os.path.join(ROOT, "include")
    deps = [SRC, os.path.join(csrc, "scene_layout.h"), os.path.join(inc, "polaris_math.h"), os.path.join(inc, "polaris_types.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + inc, "-I" + csrc, SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.lg_record_floats.restype = C.c_uint32
    lib.lg_pack.restype = None
    assert lib.lg_record_floats() == GEO
    return lib


def soup(seed):
    """Four triangles: vertices and normals [12][4] (the pad lane is not zero: it must not reach a record), uvs [12][2]."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-3, 3, (12, 4)).astype(F), rng.uniform(-1, 1, (12, 4)).astype(F), rng.uniform(0, 1, (12, 2)).astype(F))


def emissives():
    ems = np.zeros(3, T.EMISSIVE)
    # 1. an area light with an identity transform
    ems[0] = (np.eye(4, dtype=F).T.ravel(), F(0.37), 1, 5, T.EMISSIVE_AREA)
    # 2. no area light: its record is not touched
    ems[1] = (np.eye(4, dtype=F).T.ravel(), F(1.0), 0, 6, T.EMISSIVE_ENVIRONMENT)
    # 3. an area light whose transform rotates (about a skew axis), scales non-uniformly and translates
    axis = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    a, K = 0.9, np.array([[0, 0.5, 2.0], [-0.5, 0, -1.0], [-2.0, 1.0, 0]]) / np.linalg.norm([1.0, 2.0, -0.5])
    assert np.allclose(K @ axis, 0)
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag([0.5, 3.0, 1.25])
    M[:3, 3] = [7.0, -2.5, 0.125]
    ems[2] = (M.T.astype(F).ravel(), F(2.5), 3, 7, T.EMISSIVE_AREA)   # column major: m[4 c + r]
    return ems


def pack(tool, ems, vertices, normals, uvs, geo):
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    tool.lg_pack(ptr(ems), C.c_uint32(len(ems)), ptr(vertices), ptr(normals), ptr(uvs), ptr(geo))
    return geo


def restated(em, vertices, normals, uvs, before):
    """The record of area light `em` over `before`, every operation an IEEE binary32 one (numpy float32 scalars), in the order of
    scene_layout.h.  normals / uvs None: those floats stay."""
    g = before.copy()
    off = 3 * int(em["tri_index"])
    for v in range(3):
        g[4 * v:4 * v + 3] = vertices[off + v, :3]
        if normals is not None:
            g[12 + 4 * v:12 + 4 * v + 3] = normals[off + v, :3]
        if uvs is not None:
            g[24 + 2 * v:24 + 2 * v + 2] = uvs[off + v]
    m = [F(x) for x in em["transform"]]

    def mul4x1(p):   # util/transform.cl:9-16: column-major 4x4 times (p, 1), products added left to right
        return [((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r] for r in range(3)]

    v0 = [F(g[k]) for k in range(3)]
    d1 = [F(g[4 + k]) - v0[k] for k in range(3)]
    d2 = [F(g[8 + k]) - v0[k] for k in range(3)]
    tv0, te1, te2 = mul4x1(v0), mul4x1(d1), mul4x1(d2)
    cx = te1[1] * te2[2] - te1[2] * te2[1]
    cy = te1[2] * te2[0] - te1[0] * te2[2]
    cz = te1[0] * te2[1] - te1[1] * te2[0]
    inv_len = F(1.0) / np.sqrt((cx * cx + cy * cy) + cz * cz)
    assert all(type(x) is F for x in (*tv0, *te1, *te2, cx, cy, cz, inv_len))   # (nothing was promoted to double on the way)
    g[32:35], g[36:39], g[40:43] = tv0, te1, te2
    g[44:47] = [cx * inv_len, cy * inv_len, cz * inv_len]
    g[30] = F(1.0) / F(em["area"])
    return g


def test_packed_records_equal_the_float32_restatement_bit_for_bit(tool):
    ems, (vertices, normals, uvs) = emissives(), soup(1)
    geo = pack(tool, ems, vertices, normals, uvs, np.zeros((3, GEO), F))
    for e in (0, 2):
        want = restated(ems[e], vertices, normals, uvs, np.zeros(GEO, F))
        assert np.array_equal(bits(geo[e]), bits(want)), (e, geo[e], want)
        assert np.isfinite(geo[e]).all() and abs(float(np.linalg.norm(geo[e, 44:47])) - 1.0) < 1e-6
    assert not bits(geo[1]).any(), "the record of an emissive that is no area light stays zero"
    assert not np.array_equal(geo[2, 32:35], geo[2, 0:3])   # (the third light's transform does something)
    assert np.array_equal(bits(geo[0, 32:35]), bits(geo[0, 0:3]))   # (the identity does nothing: x * 1 + y * 0 + z * 0 + 0)
    # packing from the same arrays twice gives identical bytes
    again = pack(tool, ems, vertices, normals, uvs, geo.copy())
    assert again.tobytes() == geo.tobytes()
    assert pack(tool, ems, vertices, normals, uvs, np.zeros((3, GEO), F)).tobytes() == geo.tobytes()


def test_repacking_without_normals_and_uvs_keeps_them(tool):
    """What update_vertices does with normals = NULL: floats 12-29 (normals, uvs) stay, 0-11 and the derived floats follow the new vertices."""
    ems, (vertices, normals, uvs) = emissives(), soup(1)
    first = pack(tool, ems, vertices, normals, uvs, np.zeros((3, GEO), F))
    moved = soup(2)[0]
    got = pack(tool, ems, moved, None, None, first.copy())
    for e in (0, 2):
        assert np.array_equal(bits(got[e, 12:30]), bits(first[e, 12:30]))
        assert not np.array_equal(got[e, 0:12], first[e, 0:12]) and not np.array_equal(got[e, 32:47], first[e, 32:47])
        assert np.array_equal(bits(got[e]), bits(restated(ems[e], moved, None, None, first[e])))
        assert np.array_equal(bits(got[e, 0:12].reshape(3, 4)[:, :3]), bits(moved[3 * int(ems[e]["tri_index"]):][:3, :3]))
    assert not bits(got[1]).any()
    # new normals without new uvs: only the uvs stay
    normals2 = soup(3)[1]
    got = pack(tool, ems, moved, normals2, None, first.copy())
    for e in (0, 2):
        assert np.array_equal(bits(got[e]), bits(restated(ems[e], moved, normals2, None, first[e])))
        assert np.array_equal(bits(got[e, 24:30]), bits(first[e, 24:30])) and not np.array_equal(got[e, 12:24], first[e, 12:24])
