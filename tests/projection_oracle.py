"""The orthographic and equirectangular ray generators (polaris_hip_set_projection) restated in numpy:
k_generate_proj<kind>'s arithmetic and the G-buffer's centre ray, float32, every operation rounded once in the order the kernels write it.

The camera PRNG comes from oracle.random (one draw per ray: the sub-pixel offset), np.sqrt stands for pm_sqrt (both correctly rounded)
and the sine and cosine bits come from the oracle's build of polaris_math.h through Oracle.builtins, as in lens_oracle.py.  Nothing
here reads the library under test.  The inverse (tp_project: pm_atan2) has no numpy restatement: the tests call the header's own
through the host library (polaris_amd.host_api.projection_project).
"""
from __future__ import annotations

import numpy as np

import gbuffer_oracle as GO
import lens_oracle as LO
from polaris_amd import ctypes_api as T

F = np.float32
FLT_MAX = LO.FLT_MAX
ORTHOGRAPHIC, EQUIRECTANGULAR = T.PROJECTION_ORTHOGRAPHIC, T.PROJECTION_EQUIRECTANGULAR


class Projection:
    """PolarisProjectionParams as float32 numbers."""

    def __init__(self, kind, axis, right, up, half_width=0.0, half_height=0.0, lon_range=0.0, lat_range=0.0):
        self.kind = int(kind)
        self.axis, self.right, self.up = (np.asarray(x, F).reshape(3) for x in (axis, right, up))
        self.half_width, self.half_height, self.lon_range, self.lat_range = F(half_width), F(half_height), F(lon_range), F(lat_range)

    @classmethod
    def from_params(cls, p: T.ProjectionParams):
        return cls(p.kind, list(p.axis), list(p.right), list(p.up), p.half_width, p.half_height, p.lon_range, p.lat_range)

    def params(self) -> T.ProjectionParams:
        return T.projection_params(self.kind, self.axis, self.right, self.up, self.half_width, self.half_height, self.lon_range, self.lat_range)


def turned_basis(frustum, degrees=(23.0, -11.0, 7.0)):
    """(axis, right, up) float32: the frustum's view basis turned about its three vectors in turn (float64, rounded once), so that no
    entry is 0 or -0 and none of the three is a world axis."""
    axis, right, up, _ = T.projection_from_frustum(frustum)
    a, r, u = (x.astype(np.float64) for x in (axis, right, up))

    def turn(p, q, deg):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        return c * p + s * q, c * q - s * p

    a, r = turn(a, r, degrees[0])
    a, u = turn(a, u, degrees[1])
    r, u = turn(r, u, degrees[2])
    out = tuple(x.astype(F) for x in (a, r, u))
    assert all((x != 0).all() for x in out)
    return out


def _project(proj: Projection, eye, tx, ty, oracle):
    """(origins, directions) (N, 3) of the rays at the frame coordinates (tx, ty): temporal.h's tp_proj_ray."""
    eye = np.asarray(eye, F).reshape(3)
    ax, rt, up = proj.axis, proj.right, proj.up
    n = tx.size
    if proj.kind == ORTHOGRAPHIC:
        sx, sy = F(2) * tx - F(1), F(1) - F(2) * ty
        a, b = sx * proj.half_width, sy * proj.half_height
        o = np.stack([(eye[i] + rt[i] * a) + up[i] * b for i in range(3)], axis=1)
        d = np.broadcast_to(ax, (n, 3)).copy()
    else:
        lon, lat = (tx - F(0.5)) * proj.lon_range, (F(0.5) - ty) * proj.lat_range
        cl, sl = LO._sincos(oracle, lat.astype(F))
        co, so = LO._sincos(oracle, lon.astype(F))
        a, b = cl * co, cl * so
        e = [(ax[i] * a + rt[i] * b) + up[i] * sl for i in range(3)]
        inv = F(1) / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        d = np.stack([e[i] * inv for i in range(3)], axis=1)
        o = np.broadcast_to(eye, (n, 3)).copy()
    assert o.dtype == F and d.dtype == F
    return o, d


def sample_coords(oracle, W: int, H: int, block_y: int, rows: int, seed: int, paths=None):
    """(tx, ty) of every path of the block: camera_direction_from's first four lines (the tent-filtered offset of the camera stream's
    first draw)."""
    idx = LO._paths(W, rows, paths)
    s0, _ = LO.camera_draws(oracle, W, rows, seed, paths)
    gx, gy = (idx % W).astype(F), (idx // W + block_y).astype(F)
    with np.errstate(invalid="ignore"):
        tent = lambda s: np.where(s < F(0.5), np.sqrt(F(2) * s) - F(0.5), F(1.5) - np.sqrt(F(2) - F(2) * s))  # noqa: E731
        ox, oy = tent(s0[:, 0]).astype(F), tent(s0[:, 1]).astype(F)
    return ((gx + ox) * (F(1) / F(W))).astype(F), ((gy + oy) * (F(1) / F(H))).astype(F)


def projection_rays(oracle, eye, proj: Projection, W: int, H: int, block_y: int, rows: int, seed: int, paths=None):
    """(N, 8) rays as polaris_hip_tap_primary returns them with the projection on: origin | FLT_MAX | direction | path index."""
    idx = LO._paths(W, rows, paths)
    tx, ty = sample_coords(oracle, W, H, block_y, rows, seed, paths)
    o, d = _project(proj, eye, tx, ty, oracle)
    rays = np.zeros((idx.size, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, FLT_MAX, d, idx.astype(F)
    return rays


def centre_rays(oracle, eye, proj: Projection, W: int, H: int):
    """(H * W, 8) guide rays of the G-buffer: the sub-pixel offset fixed at 0.5, no seed; origin | FLT_MAX | direction | pixel index."""
    idx = np.arange(W * H)
    tx = (((idx % W).astype(F) + F(0.5)) * (F(1) / F(W))).astype(F)
    ty = (((idx // W).astype(F) + F(0.5)) * (F(1) / F(H))).astype(F)
    o, d = _project(proj, eye, tx, ty, oracle)
    rays = np.zeros((idx.size, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, FLT_MAX, d, idx.astype(F)
    return rays


def scene_extent(sc) -> float:
    lo, hi = sc.bvh_nodes["min"].min(axis=0).astype(np.float64), sc.bvh_nodes["max"].max(axis=0).astype(np.float64)
    return float((hi - lo).max())


def scene_projection(sc, kind, turned=True, lon_range=2.0 * np.pi, lat_range=np.pi) -> Projection:
    """A projection for the scene's camera: an orthographic window as high as the scene's extent, or the panorama, on the frustum's
    basis (turned: tilted a little, no -0 entry)."""
    axis, right, up, aspect = T.projection_from_frustum(sc.frustum)
    if turned:
        axis, right, up = turned_basis(sc.frustum, (9.0, -6.0, 4.0))
    half = 0.5 * scene_extent(sc)
    if kind == ORTHOGRAPHIC:
        return Projection(kind, axis, right, up, half_width=half * aspect, half_height=half)
    return Projection(kind, axis, right, up, lon_range=lon_range, lat_range=lat_range)


def gbuffer(oracle, sc, rays, W: int, H: int):
    """(guide, albedo): the (H, W, 4) planes of the G-buffer from the given guide rays (centre_rays above): gbuffer_oracle.gbuffer's
    statement -- closest hit from oracle.intersect, surfaceInit, the material walk with the PRNG state (p, p) -- on other rays.  GUIDE t
    is the hit's ray parameter, which under the orthographic camera is the distance along the axis."""
    hit, wuvt, it = oracle.intersect(sc, rays)
    guide = np.zeros((H * W, 4), F)
    guide[:, 3] = FLT_MAX
    albedo = np.ones((H * W, 4), F)
    albedo[:, 3] = GO.LEAF_MISS.view(F)
    for i in np.nonzero(hit)[0]:
        tri = int(it[i, 1])
        bu, bv = wuvt[i, 1], wuvt[i, 2]
        bw = F(1) - (bu + bv)
        o = 3 * tri
        a, b, c = sc.normals[o], sc.normals[o + 1], sc.normals[o + 2]
        n = np.array([bw * a[k] + bu * b[k] + bv * c[k] for k in range(3)], F)
        n = n * (F(1) / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]))
        ua, ub, uc = sc.uvs[o], sc.uvs[o + 1], sc.uvs[o + 2]
        uv = np.array([bw * ua[k] + bu * ub[k] + bv * uc[k] for k in range(2)], F)
        root = int(sc.material_index[tri])
        m = oracle.material_probe(sc, root, n, uv, np.array([i, i], np.uint32), 0)
        typ = int(m[0:1].view(np.int32)[0])
        guide[i, :3], guide[i, 3] = m[3:6], wuvt[i, 3]
        albedo[i, 3] = m[0:1].view(F)[0]
        if typ in (T.BXDF_DIFFUSE, T.BXDF_CONDUCTOR, T.BXDF_ROUGH_CONDUCTOR):
            kcol = m[12:15]
            leaf = GO._find_leaf(sc.material_nodes, root, typ, m[12:15], m[15:18])
            if int(leaf["tex"]) != -1:
                kcol = oracle.tex_probe(sc.texture_meta, sc.texture_data, int(leaf["tex"]), uv)[:3]
            albedo[i, :3] = np.clip(m[6:9] * kcol, F(0), F(1))
    return guide.reshape(H, W, 4), albedo.reshape(H, W, 4)
