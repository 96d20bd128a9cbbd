"""An independent numpy statement of the variance estimate and the variance-guided a-trous filter, and
engineered planes for them.

Written from the algorithm's statement with whole-frame arrays and shifted views, float32 in the statement's order of operations
with numpy's exp and sqrt.  It shares no code with polaris_amd/csrc/variance.h, which both the kernels and polaris_host_variance /
polaris_host_denoise_variance include.
"""
from __future__ import annotations

import numpy as np

from gbuffer_oracle import filtered_mask, leaf_word, random_planes
from polaris_amd import ctypes_api as T

F = np.float32
H1 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
G1 = [F(0.25), F(0.5), F(0.25)]


def lum(c):
    """Rec. 709 luminance of (..., 3), (0.2126 r + 0.7152 g) + 0.0722 b."""
    c = np.asarray(c, F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def moments_of_samples(samples):
    """(acc rgb | sum L^2) of a list of (H, W, >=3) per-sample radiance planes, added in ascending order in float32."""
    acc = np.zeros(samples[0].shape[:2] + (4,), F)
    for x in samples:
        acc[..., :3] += np.asarray(x, F)[..., :3]
        lx = lum(x[..., :3])
        acc[..., 3] += lx * lx
    return acc


def _taps(R, W, dy, dx):
    ys, xs = np.mgrid[0:R, 0:W]
    yj, xj = ys + dy, xs + dx
    ok = (yj >= 0) & (yj < R) & (xj >= 0) & (xj < W)
    return ok, np.clip(yj, 0, R - 1), np.clip(xj, 0, W - 1)


def _wn_wz(n, t, yj, xj, normal_power_log2, depth_scale):
    nj = n[yj, xj]
    w = np.maximum(F(0), n[..., 0] * nj[..., 0] + n[..., 1] * nj[..., 1] + n[..., 2] * nj[..., 2])
    for _ in range(normal_power_log2):
        w = w * w
    if depth_scale:
        w = w * np.exp(-np.abs(t - t[yj, xj]) / (F(depth_scale) * t))
    return w


def variance(frame_acc, samples, guide, albedo, *, temporal=None, prior2=None, block_y=0, block_h=None, normal_power_log2=5, sigma_depth=0.1,
             min_samples=4, sigma_variance=None):
    """The VARIANCE plane (M1 | M2 | n_eff | v) of the rows [block_y, block_y + block_h) (other rows zero); sigma_variance plays no
    part in it (accepted so that one parameter set serves both functions)."""
    H, W = frame_acc.shape[:2]
    y0, y1 = block_y, block_y + (H - block_y if block_h is None else block_h)
    rows = slice(y0, y1)
    R = y1 - y0
    n = F(samples)
    weight = F(1.0 / float(F(samples)))
    acc = frame_acc[rows].astype(F)
    c = acc[..., :3] * weight if temporal is None else temporal[rows, :, :3].astype(F)
    m1 = lum(c)
    m2 = acc[..., 3] * weight
    ne = np.full((R, W), n, F)
    if prior2 is not None:
        m = prior2[rows, :, 3].astype(F)
        h2 = prior2[rows, :, 0].astype(F)
        has = m > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            m2 = np.where(has, (acc[..., 3] + m * h2) / (n + m), m2)
        ne = np.where(has, n + m, ne)
    filt = filtered_mask(albedo[rows])
    g = guide[rows].astype(F)
    nrm, t = g[..., :3], g[..., 3]
    per_pixel = (ne >= F(min_samples)) & (ne >= F(2))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v_pp = np.maximum(F(0), m2 - m1 * m1) / (ne - F(1))
        sw = np.zeros((R, W), F)
        s1 = np.zeros((R, W), F)
        s2 = np.zeros((R, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                ok, yj, xj = _taps(R, W, dy, dx)
                ok = ok & filt[yj, xj]
                if dx == 0 and dy == 0:
                    w = np.ones((R, W), F)
                else:
                    w = np.where(ok, _wn_wz(nrm, t, yj, xj, normal_power_log2, F(sigma_depth)), F(0))
                sw += w
                s1 += w * np.where(ok, m1[yj, xj], F(0))
                s2 += w * np.where(ok, m2[yj, xj], F(0))
        a, b = s1 / sw, s2 / sw
        v_sp = np.maximum(F(0), b - a * a) / ne
    v = np.where(filt, np.where(per_pixel, v_pp, v_sp), F(0))
    out = np.zeros((H, W, 4), F)
    out[rows] = np.stack([m1, m2, ne, v], axis=-1)
    return out


def denoise_variance(acc, weight, var, guide, albedo, *, block_y=0, block_h=None, iterations=4, normal_power_log2=5, sigma_depth=0.1,
                     sigma_variance=4.0):
    """The DENOISED plane (rgb | filtered variance) of the rows [block_y, block_y + block_h) (other rows zero)."""
    H, W = acc.shape[:2]
    y0, y1 = block_y, block_y + (H - block_y if block_h is None else block_h)
    rows = slice(y0, y1)
    R = y1 - y0
    c = acc[rows, :, :3].astype(F) * F(weight)
    filt = filtered_mask(albedo[rows])
    a = np.maximum(albedo[rows, :, :3].astype(F), F(1e-3))
    la = lum(a)
    la2 = la * la
    nrm, t = guide[rows, :, :3].astype(F), guide[rows, :, 3].astype(F)
    r = c / a
    v = var[rows, :, 3].astype(F) / la2
    np_err = np.seterr(over="ignore", invalid="ignore", divide="ignore")
    for k in range(iterations):
        s = 1 << k
        gh = np.zeros((R, W), F)
        gv = np.zeros((R, W), F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                ok, yj, xj = _taps(R, W, dy, dx)
                ok = ok & filt[yj, xj]
                h = np.where(ok, G1[dx + 1] * G1[dy + 1], F(0))
                gh += h
                gv += h * np.where(ok, v[yj, xj], F(0))
        denom = F(sigma_variance) * np.sqrt(gv / gh) + F(1e-10)
        li = lum(r)
        sw = np.zeros((R, W), F)
        ar = np.zeros((R, W, 3), F)
        sv = np.zeros((R, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                h = H1[dx + 2] * H1[dy + 2]
                ok, yj, xj = _taps(R, W, dy * s, dx * s)
                ok = ok & filt[yj, xj]
                if dx == 0 and dy == 0:
                    w = np.full((R, W), h, F)
                else:
                    w = (h * _wn_wz(nrm, t, yj, xj, normal_power_log2, F(sigma_depth) * F(s))) * np.exp(-np.abs(li - li[yj, xj]) / denom)
                    w = np.where(ok, w, F(0))
                sw += w
                ar += w[..., None] * np.where(ok[..., None], r[yj, xj], F(0))
                sv += (w * w) * np.where(ok, v[yj, xj], F(0))
        r = np.where(filt[..., None], ar / np.where(filt, sw, F(1))[..., None], r)
        v = np.where(filt, sv / np.where(filt, sw * sw, F(1)), v)
    np.seterr(**np_err)
    out = np.zeros((H, W, 4), F)
    if iterations:
        out[rows, :, :3] = np.where(filt[..., None], r * a, c)
        out[rows, :, 3] = np.where(filt, v * la2, F(0))
    else:
        out[rows, :, :3] = c
    return out


def moment_planes(rng, H, W, samples):
    """random_planes with a plausible sum of L^2: per pixel, `samples` draws around the mean (L^2 summed >= the mean's)."""
    acc, guide, albedo = random_planes(rng, H, W)
    mean = acc[..., :3] / F(samples)
    spread = (rng.random((H, W)) * 2).astype(F)
    lm = lum(mean)
    acc[..., 3] = (F(samples) * (lm * lm) * (F(1) + spread)).astype(F)
    return acc, guide, albedo


def flat_planes(H, W, samples, *, leaf=T.BXDF_DIFFUSE, a=(0.5, 0.5, 0.5)):
    """One plane facing the camera, grey albedo, zero radiance."""
    acc = np.zeros((H, W, 4), F)
    guide = np.zeros((H, W, 4), F)
    guide[..., 2] = 1
    guide[..., 3] = 2
    albedo = np.zeros((H, W, 4), F)
    albedo[..., :3] = a
    albedo[..., 3] = leaf_word(np.full((H, W), leaf))
    return acc, guide, albedo
