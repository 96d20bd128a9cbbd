"""The denoiser's G-buffer with the option "guide_specular" = N restated on the CPU oracle.

Per pixel the guide ray follows up to N delta interactions.  Every link is gbuffer_oracle.gbuffer's one hit again: the closest hit
from oracle.intersect, surfaceInit restated in float32, the material walk from oracle.material_probe with the PRNG state (p, p) and
no path flags, the albedo rule of gbuffer_oracle.gbuffer.  On a CONDUCTOR or DIELECTRIC leaf the delta direction is
oracle.bxdf_probe's sample for the pair (1, 0) and in_dir = -d, on the leaf the walk selected with the IORs the walk left; the next
ray starts at p + (n * pm_sign(n . out)) * 1e-5 and keeps `out` as it is.  With N = 0 this is gbuffer_oracle.gbuffer.
"""
from __future__ import annotations

import numpy as np

import gbuffer_oracle as G
from polaris_amd import ctypes_api as T

F = np.float32
NO_INSTANCE = np.uint32(0xFFFFFFFF)
K_EPS = F(0.00001)
DIR_BOUND = F(1024.0)


def pm_sign(x):
    """polaris_math.h pm_sign: +-1, and x itself for +-0 (0 for a NaN)."""
    x = F(x)
    return F(1) if x > 0 else (F(-1) if x < 0 else (x if x == x else F(0)))


def _surface(sc, tri, bu, bv):
    bw = F(1) - (bu + bv)
    o = 3 * tri
    blend = lambda arr, n: np.array([bw * arr[o][k] + bu * arr[o + 1][k] + bv * arr[o + 2][k] for k in range(n)], F)  # noqa: E731
    p = blend(sc.vertices, 3)
    n = blend(sc.normals, 3)
    n = n * (F(1) / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]))
    return p, n, blend(sc.uvs, 2)


def chained_gbuffer(oracle, sc, W: int, H: int, links: int):
    """(guide (H, W, 4), albedo (H, W, 4), inst (H, W) uint32, info).  info: k (H, W) the links followed (-1: the pixel ends in a
    miss), textured (H, W) a texture entered the albedo, point (H, W, 3) the final hit point, first_tri (H, W) the first link's
    triangle (-1: none) and first_type (H, W) the first link's leaf type."""
    n = W * H
    rays = G.centre_rays(sc, W, H)
    guide = np.zeros((n, 4), F)
    guide[:, 3] = G.FLT_MAX
    albedo = np.ones((n, 4), F)
    albedo[:, 3] = G.LEAF_MISS.view(F)
    inst = np.full(n, NO_INSTANCE, np.uint32)
    chain = np.full(n, -1, np.int32)
    textured = np.zeros(n, bool)
    point = np.zeros((n, 3), F)
    first_tri = np.full(n, -1, np.int32)
    first_type = np.full(n, -1, np.int32)
    A = np.ones((n, 3), F)
    Tsum = np.zeros(n, F)
    active = np.arange(n)
    for k in range(links + 1):
        if len(active) == 0:
            break
        hit, wuvt, it = oracle.intersect(sc, rays[active])
        nxt = []
        for j, i in enumerate(active):
            if not hit[j]:
                textured[i] = False                               # (the miss encoding is exact)
                continue
            tri = int(it[j, 1])
            Tsum[i] = wuvt[j, 3] if k == 0 else Tsum[i] + wuvt[j, 3]
            p, nrm, uv = _surface(sc, tri, wuvt[j, 1], wuvt[j, 2])
            root = int(sc.material_index[tri])
            m = oracle.material_probe(sc, root, nrm, uv, np.array([i, i], np.uint32), 0)
            typ = int(m[0:1].view(np.int32)[0])
            if k == 0:
                first_tri[i], first_type[i] = tri, typ
            a = np.ones(3, F)
            leaf = None
            if typ in (T.BXDF_DIFFUSE, T.BXDF_CONDUCTOR, T.BXDF_ROUGH_CONDUCTOR):
                kcol = m[12:15]
                leaf = G._find_leaf(sc.material_nodes, root, typ, m[12:15], m[15:18])
                if int(leaf["tex"]) != -1:
                    kcol = oracle.tex_probe(sc.texture_meta, sc.texture_data, int(leaf["tex"]), uv)[:3]
                    textured[i] = True
                a = np.clip(m[6:9] * kcol, F(0), F(1))
            if typ in (T.BXDF_CONDUCTOR, T.BXDF_DIELECTRIC) and k < links:
                if leaf is None:
                    leaf = G._find_leaf(sc.material_nodes, root, typ, m[12:15], m[15:18])
                node = np.array(leaf, copy=True)
                node["int_ior"], node["ext_ior"] = m[1], m[2]     # after the dispersion override
                d = rays[i, 4:7]
                out = oracle.bxdf_probe(node, sc.texture_meta, sc.texture_data, m[3:6], uv, -d, np.array([1, 0], F), m[3:6])[3:6]
                with np.errstate(invalid="ignore"):
                    bounded = bool(np.all(np.abs(out) <= DIR_BOUND))  # (False for a NaN)
                if bounded and bool(np.any(out != 0)):
                    A[i] = A[i] * a
                    nn = m[3:6]
                    s = pm_sign(nn[0] * out[0] + nn[1] * out[1] + nn[2] * out[2])
                    rays[i, 0:3] = p + (nn * s) * K_EPS
                    rays[i, 4:7] = out
                    nxt.append(i)
                    continue
            guide[i, :3] = m[3:6]
            guide[i, 3] = Tsum[i]
            albedo[i, :3] = A[i] * a
            albedo[i, 3] = m[0:1].view(F)[0]
            inst[i] = np.uint32(it[j, 0]) if k == 0 else NO_INSTANCE
            chain[i] = k
            point[i] = p
        active = np.array(nxt, np.int64)
    sh = (H, W)
    return guide.reshape(H, W, 4), albedo.reshape(H, W, 4), inst.reshape(sh), {
        "k": chain.reshape(sh), "textured": textured.reshape(sh), "point": point.reshape(H, W, 3),
        "first_tri": first_tri.reshape(sh), "first_type": first_type.reshape(sh)}


def leaf_types(albedo) -> np.ndarray:
    return np.ascontiguousarray(albedo[..., 3]).view(np.int32)


def planar_mirror_tris(sc) -> np.ndarray:
    """The triangles of scenes.mirror_room's planar mirror: every vertex lies in the plane z = MIRROR_ROOM_MIRROR[2]."""
    from polaris_amd import scenes

    z = np.asarray(sc.vertices, F)[:, 2].reshape(-1, 3)
    return np.nonzero(np.all(z == F(scenes.MIRROR_ROOM_MIRROR[2]), axis=1))[0]


def through_planar_mirror(sc, info) -> np.ndarray:
    """(H, W) bool: one link was followed, and it was the planar mirror's."""
    return (info["k"] == 1) & np.isin(info["first_tri"], planar_mirror_tris(sc))


def reprojection_eligible(sc, guide, albedo, info) -> np.ndarray:
    """The pixels of the mirror experiment: seen through the planar mirror alone, a diffuse final leaf, and not
    next to a G-buffer edge."""
    return through_planar_mirror(sc, info) & (leaf_types(albedo) == T.BXDF_DIFFUSE) & ~G.edge_mask(guide)
