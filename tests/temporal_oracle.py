"""An independent numpy statement of the temporal reprojection, and engineered planes and cameras for it.

Written from the algorithm's statement with whole-frame arrays: the projection is solved in float64 with np.linalg.solve, the taps
are gathered with fancy indexing.  It shares no code with polaris_amd/csrc/temporal.h, which both the kernels and
polaris_host_reproject include.  Besides the PRIOR it returns, per pixel, how close its tap tests came to a threshold, so that a
comparison can leave out the pixels where float32 and float64 may decide a test differently.
"""
from __future__ import annotations

import numpy as np

from gbuffer_oracle import FLT_MAX, filtered_mask, leaf_word
from polaris_amd import ctypes_api as T

F = np.float32


def centre_dirs(eye, frustum, W: int, H: int) -> np.ndarray:
    """(H, W, 3) float64 unit directions through the pixel centres (the bilinear corner blend, all four components)."""
    fr = np.asarray(frustum, np.float64).reshape(4, 4)
    tl, tr, bl, br = fr
    gy, gx = np.mgrid[0:H, 0:W]
    tx = ((gx + 0.5) / W)[..., None]
    ty = ((gy + 0.5) / H)[..., None]
    d = (tl + (bl - tl) * ty) * (1 - tx) + (tr + (br - tr) * ty) * tx
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return d[..., :3]


def projectable(frustum) -> bool:
    fr = np.asarray(frustum, np.float64).reshape(4, 4)
    tl, tr, bl, br = fr
    if np.any(fr[:, 3] != 0):
        return False
    return bool(np.linalg.norm((tl + br - tr - bl)[:3]) <= 1e-3 * np.linalg.norm((tr - tl)[:3]))


def reproject(history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, *, max_history=32,
              normal_threshold=0.9, depth_threshold=0.1):
    """(prior (H, W, 4) float64, margin (H, W) float64): margin = the smallest distance of any of the pixel's tap tests, bilinear
    positions or the mu > 0 test from its threshold (inf where none was made)."""
    H, W = guide.shape[:2]
    prior = np.zeros((H, W, 4))
    margin = np.full((H, W), np.inf)
    if not projectable(prev_frustum) or max_history == 0:
        return prior, margin
    filt = filtered_mask(albedo)
    d = centre_dirs(eye, frustum, W, H)
    t = guide[..., 3].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(eye, np.float64) + t[..., None] * d
    fr = np.asarray(prev_frustum, np.float64).reshape(4, 4)[:, :3]
    tl, tr, bl = fr[0], fr[1], fr[2]
    q = p - np.asarray(prev_eye, np.float64)
    ys, xs = np.nonzero(filt)
    if len(ys) == 0:
        return prior, margin
    qs = q[ys, xs]
    M = np.empty((len(ys), 3, 3))
    M[:, :, 0] = tr - tl
    M[:, :, 1] = bl - tl
    M[:, :, 2] = -qs
    sol = np.linalg.solve(M, np.broadcast_to(-tl, (len(ys), 3))[..., None])[..., 0]
    u, v, mu = sol[:, 0], sol[:, 1], sol[:, 2]
    dist = np.linalg.norm(qs, axis=-1)
    x, y = u * W - 0.5, v * H - 0.5
    mg = np.abs(mu) / (1 + np.abs(mu))
    ok = (mu > 0) & (x > -1) & (x < W) & (y > -1) & (y < H)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    mg = np.minimum(mg, np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)))
    n_i = guide[ys, xs, :3].astype(np.float64)
    leaf_i = np.ascontiguousarray(albedo[ys, xs, 3]).view(np.uint32)
    hleaf = np.ascontiguousarray(prev_albedo[..., 3]).view(np.uint32)
    sw = np.zeros(len(ys))
    acc = np.zeros((len(ys), 4))
    for k in range(4):
        xx = np.where(ok, x0, 0).astype(np.int64) + (k & 1)
        yy = np.where(ok, y0, 0).astype(np.int64) + (k >> 1)
        w = (fx if k & 1 else 1 - fx) * (fy if k >> 1 else 1 - fy)
        inside = ok & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
        c = history[yc, xc].astype(np.float64)
        g = prev_guide[yc, xc].astype(np.float64)
        dot = np.sum(n_i * g[:, :3], axis=-1)
        with np.errstate(invalid="ignore"):
            dz = np.abs(g[:, 3] - dist) - depth_threshold * dist
        valid = inside & (c[:, 3] > 0) & np.all(np.isfinite(c[:, :3]), axis=-1) & (hleaf[yc, xc] == leaf_i) & \
            (dot >= normal_threshold) & (dz <= 0)
        near = inside & (c[:, 3] > 0) & np.all(np.isfinite(c[:, :3]), axis=-1) & (hleaf[yc, xc] == leaf_i)
        mg = np.where(near, np.minimum(mg, np.minimum(np.abs(dot - normal_threshold), np.abs(np.nan_to_num(dz, nan=1.0)) / np.maximum(dist, 1e-30))), mg)
        sw += np.where(valid, w, 0)
        acc += np.where(valid[:, None], w[:, None] * np.where(valid[:, None], c, 0), 0)
    has = sw > 0
    out = np.zeros((len(ys), 4))
    out[has] = acc[has] / sw[has, None]
    out[has, 3] = np.minimum(out[has, 3], max_history)
    out[~has] = 0
    prior[ys, xs] = out
    margin[ys, xs] = mg
    return prior, margin


def combine(frame_acc, prior, accumulated: int, spp: int) -> np.ndarray:
    """The TEMPORAL plane in float64: (acc + m h) / (n + m) | n + m where m > 0, acc / n | n elsewhere."""
    n = accumulated + spp
    a = frame_acc.astype(np.float64)
    m = prior[..., 3:4].astype(np.float64)
    out = np.empty(a.shape)
    out[..., :3] = np.where(m > 0, (a[..., :3] + m * prior[..., :3]) / (n + m), a[..., :3] / n)
    out[..., 3] = np.where(m[..., 0] > 0, n + m[..., 0], n)
    return out


# ---- engineered cameras and planes ---------------------------------------------------------------------------------------
def pinhole(eye, look=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov_deg=45.0, aspect=1.0):
    """(eye (3,), frustum (4, 4)): eye-relative corner directions TL, TR, BL, BR on the image plane at distance 1, w = 0."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(look, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    h = np.tan(np.radians(fov_deg) / 2)
    w = h * aspect
    corners = [f - r * w + u * h, f + r * w + u * h, f - r * w - u * h, f + r * w - u * h]
    fr = np.zeros((4, 4), F)
    fr[:, :3] = np.asarray(corners, F)
    return eye.astype(F), fr


def trace_planes(eye, frustum, W, H, planes):
    """First-hit guide / albedo of a camera over a list of one-sided rectangles dict(n, d, lo, hi, leaf, albedo):
    points x with n . x = d inside the box [lo, hi].  float64 arithmetic rounded to float32 at the end."""
    dirs = centre_dirs(eye, frustum, W, H)
    e = np.asarray(eye, np.float64)
    best = np.full((H, W), np.inf)
    guide = np.zeros((H, W, 4), F)
    guide[..., 3] = FLT_MAX
    albedo = np.ones((H, W, 4), F)
    albedo[..., 3] = leaf_word(np.full((H, W), -1))
    for pl in planes:
        n = np.asarray(pl["n"], np.float64)
        n = n / np.linalg.norm(n)
        den = dirs @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (pl["d"] - e @ n) / den
        x = e + t[..., None] * dirs
        lo, hi = np.asarray(pl["lo"]), np.asarray(pl["hi"])
        hit = (t > 1e-6) & np.all((x >= lo - 1e-9) & (x <= hi + 1e-9), axis=-1) & (t < best)
        best = np.where(hit, t, best)
        guide[hit, :3] = np.where((den[hit] < 0)[:, None], n, -n).astype(F)   # (facing the camera)
        guide[hit, 3] = t[hit].astype(F)
        albedo[hit, :3] = np.asarray(pl.get("albedo", (0.5, 0.5, 0.5)), F)
        albedo[hit, 3] = leaf_word(np.full(int(hit.sum()), pl.get("leaf", T.BXDF_DIFFUSE)))
    return guide, albedo


WALL = dict(n=(0, 0, 1), d=-4.0, lo=(-50, -50, -4.0), hi=(50, 50, -4.0))
