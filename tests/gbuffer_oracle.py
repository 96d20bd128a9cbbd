"""The denoiser's first-hit G-buffer restated on the CPU oracle, and an independent numpy statement of its filter.

G-buffer (include/polaris_hip.h, POLARIS_AOV_GUIDE / _ALBEDO): one ray per pixel through the pixel centre (k_generate's
arithmetic with the sub-pixel offset 0.5), its closest hit from oracle.intersect, surfaceInit restated here, and the material
walk from oracle.material_probe with the PRNG state (p, p), p = gy * W + gx, and no path flags.  Textured albedo comes from
oracle.tex_probe of the selected leaf, found in the triangle's material tree by its type, k and t.

Filter: written from the algorithm's statement with whole-frame numpy arrays -- it shares no code with
polaris_amd/csrc/denoise.h, which both the kernel and polaris_host_denoise include.
"""
from __future__ import annotations

import numpy as np

from polaris_amd import ctypes_api as T

F = np.float32
FLT_MAX = F(3.402823466e38)
LEAF_MISS = np.uint32(0xFFFFFFFF)


def centre_rays(sc, W: int, H: int) -> np.ndarray:
    """(H*W, 8) rays: eye, FLT_MAX, unit direction through the pixel centre, 0 (camera.cl's arithmetic, offset 0.5)."""
    fr = np.asarray(sc.frustum, F).reshape(4, 4)
    tl, tr, bl, br = fr[0], fr[1], fr[2], fr[3]
    gy, gx = np.mgrid[0:H, 0:W]
    tx = (gx.reshape(-1).astype(F) + F(0.5)) * (F(1) / F(W))
    ty = (gy.reshape(-1).astype(F) + F(0.5)) * (F(1) / F(H))
    mix = lambda a, b, t: a + (b - a) * t  # noqa: E731
    d = [mix(mix(tl[c], bl[c], ty), mix(tr[c], br[c], ty), tx) for c in range(4)]
    inv = F(1) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    rays = np.zeros((H * W, 8), F)
    rays[:, 0:3] = np.asarray(sc.eye, F)
    rays[:, 3] = FLT_MAX
    for c in range(3):
        rays[:, 4 + c] = d[c] * inv
    return rays


def _find_leaf(nodes, root: int, typ: int, k, t):
    """The leaf under `root` with this type, k and t (the material probe names the selected leaf by them)."""
    stack, seen = [root], set()
    while stack:
        i = stack.pop()
        if i in seen or i < 0 or i >= len(nodes):
            continue
        seen.add(i)
        nd = nodes[i]
        ty = int(nd["type"])
        if ty >= T.OP_MIX:
            stack.append(int(nd["left_child"]))
            if ty in (T.OP_MIX, T.OP_MIX_MAP):
                stack.append(int(nd["right_child"]))
            continue
        if ty == typ and np.array_equal(nd["k"][:3].view(np.uint32), np.asarray(k, F).view(np.uint32)) and \
                np.array_equal(nd["t"][:3].view(np.uint32), np.asarray(t, F).view(np.uint32)):
            return nd
    raise AssertionError(f"no leaf of type {typ} under material node {root}")


def gbuffer(oracle, sc, W: int, H: int):
    """(guide, albedo, info): (H, W, 4) float32 planes as the device computes them, and per-pixel details for the tests
    (tint (H, W, 3), textured (H, W) bool: the albedo came from a texture)."""
    rays = centre_rays(sc, W, H)
    hit, wuvt, it = oracle.intersect(sc, rays)
    guide = np.zeros((H * W, 4), F)
    guide[:, 3] = FLT_MAX
    albedo = np.ones((H * W, 4), F)
    albedo[:, 3] = LEAF_MISS.view(F)
    tint = np.ones((H * W, 3), F)
    textured = np.zeros(H * W, bool)
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
        guide[i, :3] = m[3:6]
        guide[i, 3] = wuvt[i, 3]
        tint[i] = m[6:9]
        albedo[i, 3] = m[0:1].view(F)[0]
        if typ in (T.BXDF_DIFFUSE, T.BXDF_CONDUCTOR, T.BXDF_ROUGH_CONDUCTOR):
            kcol = m[12:15]
            leaf = _find_leaf(sc.material_nodes, root, typ, m[12:15], m[15:18])
            if int(leaf["tex"]) != -1:
                kcol = oracle.tex_probe(sc.texture_meta, sc.texture_data, int(leaf["tex"]), uv)[:3]
                textured[i] = True
            albedo[i, :3] = np.clip(m[6:9] * kcol, F(0), F(1))
    return guide.reshape(H, W, 4), albedo.reshape(H, W, 4), {"tint": tint.reshape(H, W, 3), "textured": textured.reshape(H, W)}


LEAVES = np.array([T.BXDF_DIFFUSE, T.BXDF_CONDUCTOR, T.BXDF_ROUGH_CONDUCTOR, T.BXDF_DIELECTRIC, T.BXDF_EMISSIVE, -1], np.int32)


def leaf_word(types):
    return np.asarray(types, np.int32).view(F)


def random_planes(rng, H, W):
    """Radiance sums, a guide of mostly aligned normals with depth steps, albedo with dark channels, misses and emitters."""
    acc = np.zeros((H, W, 4), F)
    acc[..., :3] = (rng.random((H, W, 3)) ** 3 * 40).astype(F)
    n = np.array([0.2, 0.3, 1.0]) + 0.35 * rng.standard_normal((H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    guide = np.zeros((H, W, 4), F)
    guide[..., :3] = n
    guide[..., 3] = (1.0 + rng.random((H, W)) * 0.2 + (np.arange(W) >= W // 2) * 1.5).astype(F)
    albedo = np.zeros((H, W, 4), F)
    albedo[..., :3] = rng.random((H, W, 3))
    albedo[..., :3][rng.random((H, W, 3)) < 0.05] = 0.0
    leaves = LEAVES[rng.choice(len(LEAVES), size=(H, W), p=[0.55, 0.1, 0.1, 0.1, 0.05, 0.1])]
    albedo[..., 3] = leaf_word(leaves)
    miss = leaves == -1
    guide[miss] = [0, 0, 0, FLT_MAX]
    albedo[miss, :3] = 1.0
    return acc, guide, albedo


def filtered_mask(albedo: np.ndarray) -> np.ndarray:
    leaf = np.ascontiguousarray(albedo[..., 3]).view(np.uint32)
    return (leaf != LEAF_MISS) & (leaf != T.BXDF_EMISSIVE)


def atrous(frame_acc, weight, guide, albedo, *, block_y=0, block_h=None, iterations=4, normal_power_log2=5, sigma_depth=0.1,
           sigma_luminance=4.0) -> np.ndarray:
    """The filter of DESIGN.md section 10 on the rows [block_y, block_y + block_h): returns the (H, W, 3) result of those rows
    (other rows zero).  float32 in the statement's order of operations, numpy's exp for pm_exp."""
    H, W = frame_acc.shape[:2]
    y0, y1 = block_y, block_y + (H - block_y if block_h is None else block_h)
    c = frame_acc[y0:y1, :, :3].astype(F) * F(weight)
    filt = filtered_mask(albedo[y0:y1])
    a = np.maximum(albedo[y0:y1, :, :3].astype(F), F(1e-3))
    n = guide[y0:y1, :, :3].astype(F)
    t = guide[y0:y1, :, 3].astype(F)
    r = c / a
    h1 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
    R = y1 - y0
    m = lambda x: x / (x + F(1))  # noqa: E731
    ys, xs = np.mgrid[0:R, 0:W]
    np_err = np.seterr(over="ignore", invalid="ignore", divide="ignore")   # (the masked taps of misses: t = FLT_MAX)
    for k in range(iterations):
        s = 1 << k
        wsum = np.zeros((R, W), F)
        acc = np.zeros((R, W, 3), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                h = h1[dx + 2] * h1[dy + 2]
                # tap j = i + (dx, dy) * s, for every centre i at once (invalid taps weigh 0)
                yj, xj = ys + dy * s, xs + dx * s
                ok = (yj >= 0) & (yj < R) & (xj >= 0) & (xj < W)
                yj, xj = np.clip(yj, 0, R - 1), np.clip(xj, 0, W - 1)
                ok &= filt[yj, xj]
                rj = r[yj, xj]
                if dx == 0 and dy == 0:
                    w = np.full((R, W), h, F)
                else:
                    nj = n[yj, xj]
                    wn = np.maximum(F(0), n[..., 0] * nj[..., 0] + n[..., 1] * nj[..., 1] + n[..., 2] * nj[..., 2])
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    w = h * wn
                    if sigma_depth:
                        w = w * np.exp(-np.abs(t - t[yj, xj]) / ((F(sigma_depth) * F(s)) * t))
                    if sigma_luminance:
                        d = m(r) - m(rj)
                        sq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
                        w = w * np.exp(-sq / ((F(sigma_luminance) * F(sigma_luminance)) * F(2.0 ** -k)))
                w = np.where(ok, w, F(0))
                wsum += w
                acc += w[..., None] * np.where(ok[..., None], rj, F(0))
        r = np.where(filt[..., None], acc / np.where(filt, wsum, F(1))[..., None], r)
    np.seterr(**np_err)
    out = np.zeros((H, W, 3), F)
    out[y0:y1] = np.where(filt[..., None], r * a, c) if iterations else c
    return out


def edge_mask(guide: np.ndarray) -> np.ndarray:
    """Pixels next to a G-buffer edge: to a 4-neighbour the normals' dot is < 0.9 or the depth jumps by more than 10 %
    (a miss next to a hit counts as an edge)."""
    H, W = guide.shape[:2]
    n = guide[..., :3].astype(np.float64)
    t = guide[..., 3].astype(np.float64)
    hit = guide[..., 3] < FLT_MAX
    e = np.zeros((H, W), bool)
    for dy, dx in ((0, 1), (1, 0)):
        a = (slice(0, H - dy), slice(0, W - dx))
        b = (slice(dy, H), slice(dx, W))
        both = hit[a] & hit[b]
        dot = np.sum(n[a] * n[b], axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            jump = np.abs(t[a] - t[b]) > 0.1 * np.minimum(t[a], t[b])
        edge = (hit[a] != hit[b]) | (both & ((dot < 0.9) | jump))
        e[a] |= edge
        e[b] |= edge
    return e
