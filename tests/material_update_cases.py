"""The (base, substituted, args) triples of the material-update tests (tests/test_material_update_cpu.py, tests/test_gpu_material_update.py).

Every case is a base scene, the arguments of polaris_hip_update_materials / polaris_hip_update_texture, and
scenes.with_materials(base, **args): the scene the update must make of an uploaded `base`.  args holds `nodes`,
`material_index`, `scene_diffuse`, `emissive_mat_nodes` (None: the call passes NULL) and `textures` ({index: texels}, one
update_texture each).  Node numbers of the Cornell box are those scenes.cornell_box("layered") hands out, asserted below.
"""
import dataclasses
import functools

import numpy as np

from polaris_amd import ctypes_api as T
from polaris_amd import scenes

F32 = np.float32
# cornell_box("layered"): the order of its MaterialTable calls
WHITE, RED, GREEN, LIGHT, FLOOR, BACK_LEAF, BACK_BUMP, GOLD, TALL_LEAF, TALL_MIX, GLASS, FROSTED, MIRROR = range(13)


def leaf(type_, k=(0, 0, 0), t=(0, 0, 0), scale=0.0, int_ior=1.5, ext_ior=1.0, tex=-1, roughness_tex=-1, right_child=-1):
    mt = scenes.MaterialTable()
    mt._node(type_, k=k, t=t, scale=scale, int_ior=int_ior, ext_ior=ext_ior, tex=tex, roughness_tex=roughness_tex, right_child=right_child)
    return mt.nodes[0]


def operator(type_, left, right=-1, tex=-1, weight=0.0):
    mt = scenes.MaterialTable()
    mt._node(type_, left_child=left, right_child=right, tex=tex, k=(weight,))
    return mt.nodes[0]


def cornell():
    sc = scenes.cornell_box("layered")
    n = sc.material_nodes
    assert sc.num_triangles == 808 and len(n) == 13 and n["type"][LIGHT] == T.BXDF_EMISSIVE and n["type"][TALL_MIX] == T.OP_MIX
    assert n["type"][GOLD] == T.BXDF_ROUGH_CONDUCTOR and n["type"][BACK_BUMP] == T.OP_BUMP_MAP and n["type"][GLASS] == T.BXDF_DIELECTRIC
    return sc


def made(base, **args):
    full = dict(nodes=None, material_index=None, scene_diffuse=None, emissive_mat_nodes=None, textures=None)
    full.update(args)
    sub = scenes.with_materials(base, **full)
    if full["nodes"] is None:
        full["nodes"] = base.material_nodes.copy()
    if full["scene_diffuse"] is None:
        full["scene_diffuse"] = int(base.scene_diffuse_mat_index)
    return base, sub, full


def _recolour():
    base = cornell()
    n = base.material_nodes.copy()
    n["k"][RED][:3] = (0.1, 0.2, 0.7)
    n["k"][LIGHT][:3] = (9.0, 14.0, 16.0)
    n["scale"][LIGHT] = 1.25
    n["scale"][GOLD] = 0.15
    n["k"][TALL_MIX][0] = 0.25
    n["int_ior"][GLASS], n["ext_ior"][GLASS] = 1.33, 1.01
    n["t"][FROSTED][:3] = (0.6, 0.9, 0.95)
    return made(base, nodes=n)


def _retype():
    base = cornell()
    n = base.material_nodes.copy()
    n[GREEN] = leaf(T.BXDF_ROUGH_CONDUCTOR, k=(0.3, 0.8, 0.4), scale=0.3, int_ior=0.0)
    n[TALL_MIX] = leaf(T.BXDF_DIFFUSE, k=(0.2, 0.5, 0.7))
    return made(base, nodes=n)


def _new_emitter():
    base = cornell()
    n = base.material_nodes.copy()
    n[RED] = operator(T.OP_MIX, TALL_LEAF, LIGHT, weight=0.7)     # the left wall: mix(diffuse, the light's emissive leaf)
    return made(base, nodes=n)


def _light_off():
    base = cornell()
    n = base.material_nodes.copy()
    n[LIGHT] = leaf(T.BXDF_DIFFUSE, k=(0.7, 0.7, 0.6))
    return made(base, nodes=n, emissive_mat_nodes=base.emissives["mat_node_index"].copy())


def _reassign():
    base = scenes.many_materials_scene()
    mi = base.material_index.copy()
    rng = np.random.default_rng(5)
    pick = rng.permutation(len(mi))[:len(mi) // 3]
    mi[pick] = mi[rng.permutation(pick)]
    assert (mi != base.material_index).sum() > len(mi) // 8
    return made(base, material_index=mi)


def _textured():
    tex = scenes.textured_materials_scene()
    L8, L32, RGBA8 = 0, 1, 2
    n0 = tex.material_nodes
    spare = len(n0)                       # headroom: an operator node nothing refers to
    base = dataclasses.replace(tex, material_nodes=np.concatenate([n0, np.array([operator(T.OP_BUMP_MAP, 0, tex=L8)], dtype=T.MATERIAL_NODE)]),
                               name="materials-headroom")
    n = base.material_nodes.copy()
    rough = int(np.nonzero(n["roughness_tex"] == L32)[0][0])
    n["tex"][rough], n["roughness_tex"][rough] = n["roughness_tex"][rough], n["tex"][rough]
    mm = int(np.nonzero(n["type"] == T.OP_MIX_MAP)[0][0])
    n[mm] = operator(T.OP_MIX, int(n["left_child"][mm]), int(n["right_child"][mm]), weight=0.35)
    over = int(np.nonzero((n["type"] == T.BXDF_DIFFUSE) & (n["tex"] == 3))[0][0])       # the back wall's RGBA32F-textured leaf
    n[spare] = operator(T.OP_BUMP_MAP, over, tex=L32)
    mi = base.material_index.copy()
    mi[mi == over] = spare
    assert (mi == spare).any()
    rng = np.random.default_rng(23)
    m8, m32 = base.texture_meta[RGBA8], base.texture_meta[L32]
    assert m8["format"] == T.TEX_RGBA8 and m32["format"] == T.TEX_L32F
    paint8 = scenes.checker_rgba8(int(m8["width"]), 8, (30, 220, 60), (240, 230, 40))
    paint32 = rng.random((int(m32["height"]), int(m32["width"]))).astype(F32)
    return made(base, nodes=n, material_index=mi, textures={RGBA8: paint8, L32: paint32})


def _background():
    base = scenes.sphere_scene()
    assert base.scene_diffuse_mat_index >= 0
    return made(base, scene_diffuse=-1)


def _class_15():
    """many_materials_scene has more reach sets than classes; its dispersion nodes sort last and share class 15.  The edit turns the
    leaf under one of them into an emitter: class 15 gains the bit."""
    base = scenes.many_materials_scene()
    n = base.material_nodes.copy()
    disp = int(np.nonzero(n["type"] == T.OP_DISPERSE)[0][-1])
    n[int(n["left_child"][disp])] = leaf(T.BXDF_EMISSIVE, k=(3.0, 2.0, 1.0), scale=1.0)
    return made(base, nodes=n)


def _not_tiny():
    grid = scenes.unique_stress(64)      # 8 194 triangles: more than 2 046 slots, no meta word
    n0 = grid.material_nodes
    spare = len(n0)                       # headroom: a second surface material nothing refers to yet
    base = dataclasses.replace(grid, material_nodes=np.concatenate([n0, np.array([leaf(T.BXDF_CONDUCTOR, k=(0.9, 0.9, 0.9), int_ior=0.0)], dtype=T.MATERIAL_NODE)]),
                               name="terrain-headroom")
    assert base.num_triangles == 8194
    n = base.material_nodes.copy()
    n["k"][spare][:3] = (0.95, 0.7, 0.3)
    mi = base.material_index.copy()
    terrain = np.nonzero(mi == 0)[0]
    mi[terrain[::3]] = spare
    return made(base, nodes=n, material_index=mi)


CASES = {
    "recolour": _recolour,          # classes and mask unchanged: the records stay the base's
    "retype": _retype,              # classes change, the mask does not
    "new-emitter": _new_emitter,    # the mask gains a bit
    "light-off": _light_off,        # the mask loses a bit; emissive_mat_nodes given
    "reassign": _reassign,          # material_index only
    "textured": _textured,          # texture indices, operators, headroom, two repainted textures
    "background": _background,      # scene_diffuse_mat_index -> -1
    "class-15": _class_15,          # an emitter moves into the shared class
    "not-tiny": _not_tiny,          # more than 2 046 slots: no meta word
}
MASK_CHANGES = ("new-emitter", "light-off", "class-15")
TINY = ("recolour", "retype", "new-emitter", "light-off", "background")      # at most 2 046 slots: the tiny-scene mode is legal


@functools.lru_cache(maxsize=None)
def case(name):
    """(base, substituted, args) of a case, built once per process and shared: leave them unchanged."""
    return CASES[name]()


def apply(tr, args):
    """The case's calls on a HipTracer that holds `base`."""
    tr.update_materials(args["nodes"], args["material_index"], args["scene_diffuse"], args["emissive_mat_nodes"])
    for index, texels in (args["textures"] or {}).items():
        tr.update_texture(index, texels)
