"""The thin-lens ray generator (polaris_hip_set_lens) restated in numpy: k_generate_lens' arithmetic, float32,
every operation rounded once in the order the kernel writes it.

The camera PRNG comes from oracle.random (two draws per ray: the sub-pixel offset, then the lens point), np.sqrt stands for
pm_sqrt (both correctly rounded, as in gbuffer_oracle.py) and the sine and cosine bits come from the oracle's build of
polaris_math.h through Oracle.builtins.  Nothing here reads the library under test.
"""
from __future__ import annotations

import numpy as np

from polaris_amd import ctypes_api as T

F = np.float32
FLT_MAX = F(3.402823466e38)
PI_4, PI_2 = F(0.78539816339744830962), F(1.57079632679489661923)


class Lens:
    """PolarisLensParams as float32 numbers."""

    def __init__(self, focus_distance, axis, u, v):
        self.focus_distance = F(focus_distance)
        self.axis, self.u, self.v = (np.asarray(x, F).reshape(3) for x in (axis, u, v))

    @classmethod
    def from_frustum(cls, frustum, radius, focus_distance):
        return cls(focus_distance, *T.lens_from_frustum(frustum, radius))

    def vectors(self):
        return float(self.focus_distance), self.axis, self.u, self.v


def _paths(W: int, rows: int, paths):
    return np.arange(W * rows) if paths is None else np.asarray(paths, np.int64).reshape(-1)


def camera_draws(oracle, W: int, rows: int, seed: int, paths=None):
    """(s0, s1): the first two draws (N, 2) of the camera stream of every path of a block of `rows` rows (or of the listed path
    indices only), state (gx + seed, gy + seed) with gy counted from the block's first row (camera.cl:38)."""
    idx = _paths(W, rows, paths)
    s0, s1 = np.zeros((idx.size, 2), F), np.zeros((idx.size, 2), F)
    for k, i in enumerate(int(x) for x in idx):
        st = [(i % W + seed) & 0xFFFFFFFF, (i // W + seed) & 0xFFFFFFFF]
        st, s0[k] = oracle.random(st)
        st, s1[k] = oracle.random(st)
    return s0, s1


def pinhole_directions(sc, W: int, H: int, block_y: int, rows: int, s0, paths=None):
    """(N, 3) unit directions of k_generate: tent-filtered offset from the first draw, the bilinear corner blend, normalize over four lanes."""
    fr = np.asarray(sc.frustum, F).reshape(4, 4)
    tl, tr, bl, br = fr[0], fr[1], fr[2], fr[3]
    idx = _paths(W, rows, paths)
    gx, gy = (idx % W).astype(F), (idx // W + block_y).astype(F)
    with np.errstate(invalid="ignore"):
        tent = lambda s: np.where(s < F(0.5), np.sqrt(F(2) * s) - F(0.5), F(1.5) - np.sqrt(F(2) - F(2) * s))  # noqa: E731
        ox, oy = tent(s0[:, 0]), tent(s0[:, 1])
    tx = (gx + ox) * (F(1) / F(W))
    ty = (gy + oy) * (F(1) / F(H))
    mix = lambda a, b, t: a + (b - a) * t  # noqa: E731
    d = [mix(mix(tl[c], bl[c], ty), mix(tr[c], br[c], ty), tx) for c in range(4)]
    inv = F(1) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    return np.stack([d[0] * inv, d[1] * inv, d[2] * inv], axis=1)


def _sincos(oracle, phi):
    """pm_cos(phi), pm_sin(phi) per element, from the oracle's build of polaris_math.h."""
    words = np.ascontiguousarray(phi, F).view(np.uint32)
    uniq, inverse = np.unique(words, return_inverse=True)
    cos, sin = np.zeros(uniq.size, np.uint32), np.zeros(uniq.size, np.uint32)
    for k, w in enumerate(uniq):
        cos[k] = oracle.builtins(T.BUILTINS["cos"], first=int(w), count=1, results=True)[0][0]
        sin[k] = oracle.builtins(T.BUILTINS["sin"], first=int(w), count=1, results=True)[0][0]
    return cos.view(F)[inverse], sin.view(F)[inverse]


def disk_points(oracle, s1):
    """(lx, ly): the concentric map (Shirley and Chiu) of the second draw."""
    a, b = F(2) * s1[:, 0] - F(1), F(2) * s1[:, 1] - F(1)
    zero = (a == 0) & (b == 0)
    wide = ~zero & (np.abs(a) > np.abs(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(zero, F(0), np.where(wide, a, b))
        phi = np.where(zero, F(0), np.where(wide, PI_4 * (b / a), PI_2 - PI_4 * (a / b))).astype(F)
    cos, sin = _sincos(oracle, phi)
    return (r * cos).astype(F), (r * sin).astype(F)


def lens_rays(oracle, sc, lens: Lens, W: int, H: int, block_y: int, rows: int, seed: int, details: bool = False, paths=None):
    """(N, 8) rays as polaris_hip_tap_primary returns them with the lens on: origin | FLT_MAX | unit direction | path index.
    paths: only these path indices of the block.  details: also a dict with the pinhole direction d, the lens point (lx, ly), c = d . axis and ft."""
    idx = _paths(W, rows, paths)
    s0, s1 = camera_draws(oracle, W, rows, seed, paths)
    d = pinhole_directions(sc, W, H, block_y, rows, s0, paths)
    lx, ly = disk_points(oracle, s1)
    eye = np.asarray(sc.eye, F).reshape(3)
    ax, u, v = lens.axis, lens.u, lens.v
    c = d[:, 0] * ax[0] + d[:, 1] * ax[1] + d[:, 2] * ax[2]
    on = c > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ft = lens.focus_distance / c
        L = np.stack([lx * u[k] + ly * v[k] for k in range(3)], axis=1)
        q = np.stack([d[:, k] * ft - L[:, k] for k in range(3)], axis=1)
        inv2 = F(1) / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])
        origin = np.stack([eye[k] + L[:, k] for k in range(3)], axis=1)
        direction = q * inv2[:, None]
    rays = np.zeros((idx.size, 8), F)
    rays[:, 0:3] = np.where(on[:, None], origin, eye[None, :])
    rays[:, 3] = FLT_MAX
    rays[:, 4:7] = np.where(on[:, None], direction, d)
    rays[:, 7] = idx.astype(F)
    assert rays.dtype == F
    if details:
        return rays, {"d": d, "lx": lx, "ly": ly, "c": c, "ft": ft, "on": on}
    return rays
