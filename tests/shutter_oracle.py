"""The shutter ray generator (polaris_hip_set_shutter) restated in numpy: k_generate_shutter<LENS>'s arithmetic,
float32, every operation rounded once in the order the kernel writes it.

The camera PRNG comes from oracle.random (per ray: the sub-pixel offset, with the lens on the lens point, then the time), np.sqrt
stands for pm_sqrt and the sine and cosine bits come from the oracle's build of polaris_math.h (lens_oracle.disk_points).  Nothing
here reads the library under test.
"""
from __future__ import annotations

import numpy as np

import lens_oracle as LO

F = np.float32
FLT_MAX = LO.FLT_MAX


class Close:
    """The state at shutter close: eye1 (3,), frustum1 (4, 4) and, under a lens, the close lens (a lens_oracle.Lens)."""

    def __init__(self, eye1, frustum1, lens1: LO.Lens | None = None):
        self.eye1 = np.asarray(eye1, F).reshape(3)
        self.frustum1 = np.asarray(frustum1, F).reshape(4, 4)
        self.lens1 = lens1


def mix(a, b, t):
    """pm_mix: a + (b - a) * t, each operation rounded to float32."""
    a, b, t = F(a) if np.isscalar(a) else a.astype(F), F(b) if np.isscalar(b) else b.astype(F), t.astype(F)
    return (a + ((b - a) * t).astype(F)).astype(F)


def shutter_draws(oracle, W: int, rows: int, seed: int, lens: bool, paths=None):
    """(s0, s1, t): the draws of the camera stream of every path of a block (or of the listed paths): the sub-pixel offset (N, 2), with
    the lens on the lens point (N, 2) (else zeros, not drawn), and the .x of the NEXT draw: the ray's time (N,)."""
    idx = LO._paths(W, rows, paths)
    s0, s1, t = np.zeros((idx.size, 2), F), np.zeros((idx.size, 2), F), np.zeros(idx.size, F)
    for k, i in enumerate(int(x) for x in idx):
        st = [(i % W + seed) & 0xFFFFFFFF, (i // W + seed) & 0xFFFFFFFF]
        st, s0[k] = oracle.random(st)
        if lens:
            st, s1[k] = oracle.random(st)
        st, draw = oracle.random(st)
        t[k] = draw[0]
    return s0, s1, t


def directions(corners, W: int, H: int, block_y: int, rows: int, s0, paths=None):
    """k_generate's direction arithmetic after the first draw with PER-RAY corners: corners[j] is (N, 4) for j = TL, TR, BL, BR."""
    tl, tr, bl, br = corners
    idx = LO._paths(W, rows, paths)
    gx, gy = (idx % W).astype(F), (idx // W + block_y).astype(F)
    with np.errstate(invalid="ignore"):
        tent = lambda s: np.where(s < F(0.5), np.sqrt(F(2) * s) - F(0.5), F(1.5) - np.sqrt(F(2) - F(2) * s))  # noqa: E731
        ox, oy = tent(s0[:, 0]), tent(s0[:, 1])
    tx = (gx + ox) * (F(1) / F(W))
    ty = (gy + oy) * (F(1) / F(H))
    m = lambda a, b, t: a + (b - a) * t  # noqa: E731
    d = [m(m(tl[:, c], bl[:, c], ty), m(tr[:, c], br[:, c], ty), tx) for c in range(4)]
    assert all(x.dtype == F for x in d)
    inv = F(1) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    return np.stack([d[0] * inv, d[1] * inv, d[2] * inv], axis=1)


def shutter_rays(oracle, sc, close: Close, W: int, H: int, block_y: int, rows: int, seed: int, lens: LO.Lens | None = None, details: bool = False, paths=None):
    """(N, 8) rays as polaris_hip_tap_primary returns them with the shutter on: origin | FLT_MAX | unit direction | path index.
    lens: the OPEN lens when the lens is on (close.lens1 is then the close one).  details: also a dict with each ray's time t, the
    camera at that time (eye_t (N, 3), corners_t) and, under a lens, the lens at that time and the pinhole direction d."""
    idx = LO._paths(W, rows, paths)
    n = idx.size
    s0, s1, t = shutter_draws(oracle, W, rows, seed, lens is not None, paths)
    eye0, fr0 = np.asarray(sc.eye, F).reshape(3), np.asarray(sc.frustum, F).reshape(4, 4)
    eye_t = np.stack([mix(eye0[k], close.eye1[k], t) for k in range(3)], axis=1)
    corners_t = [np.stack([mix(fr0[j, c], close.frustum1[j, c], t) for c in range(4)], axis=1) for j in range(4)]
    d = directions(corners_t, W, H, block_y, rows, s0, paths)
    rays = np.zeros((n, 8), F)
    rays[:, 3] = FLT_MAX
    rays[:, 7] = idx.astype(F)
    det = {"t": t, "eye_t": eye_t, "corners_t": corners_t, "d": d}
    if lens is None:
        rays[:, 0:3], rays[:, 4:7] = eye_t, d
    else:
        l1 = close.lens1
        focus_t = mix(lens.focus_distance, l1.focus_distance, t)
        ax, u, v = (np.stack([mix(a[k], b[k], t) for k in range(3)], axis=1) for a, b in ((lens.axis, l1.axis), (lens.u, l1.u), (lens.v, l1.v)))
        lx, ly = LO.disk_points(oracle, s1)
        c = d[:, 0] * ax[:, 0] + d[:, 1] * ax[:, 1] + d[:, 2] * ax[:, 2]
        on = c > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ft = focus_t / c
            L = np.stack([lx * u[:, k] + ly * v[:, k] for k in range(3)], axis=1)
            q = np.stack([d[:, k] * ft - L[:, k] for k in range(3)], axis=1)
            inv2 = F(1) / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])
            origin = eye_t + L
            direction = q * inv2[:, None]
        assert origin.dtype == direction.dtype == F
        rays[:, 0:3] = np.where(on[:, None], origin, eye_t)
        rays[:, 4:7] = np.where(on[:, None], direction, d)
        det.update({"focus_t": focus_t, "axis_t": ax, "u_t": u, "v_t": v, "lx": lx, "ly": ly, "c": c, "ft": ft, "on": on})
    assert rays.dtype == F
    return (rays, det) if details else rays


# ---- the cameras the tests use (shared by test_shutter_cpu.py and test_gpu_shutter.py)

def scene_extent(sc) -> float:
    lo, hi = sc.bvh_nodes["min"].min(axis=0).astype(np.float64), sc.bvh_nodes["max"].max(axis=0).astype(np.float64)
    return float((hi - lo).max())


def close_camera(sc, shift_of_extent: float = 0.05, turn_degrees: float = 2.0):
    """(eye1 (3,), frustum1 (4, 4)) float32: the open eye moved shift_of_extent x the scene's extent along TR - TL, the corner rays
    turned turn_degrees about the up vector TL - BL (Rodrigues' formula); computed in float64, rounded once."""
    fr = np.asarray(sc.frustum, np.float64).reshape(4, 4)
    unit = lambda x: x / np.sqrt(np.dot(x, x))  # noqa: E731
    right, up = unit(fr[1, :3] - fr[0, :3]), unit(fr[0, :3] - fr[2, :3])
    eye1 = np.asarray(sc.eye, np.float64).reshape(3) + shift_of_extent * scene_extent(sc) * right
    a = np.radians(turn_degrees)
    fr1 = fr.copy()
    for j in range(4):
        x = fr[j, :3]
        fr1[j, :3] = x * np.cos(a) + np.cross(up, x) * np.sin(a) + up * np.dot(up, x) * (1 - np.cos(a))
    return eye1.astype(F), fr1.astype(F)


def no_negative_zero(*arrays) -> bool:
    """No entry is -0: pm_mix(a, a, t) = a holds for every entry (a -0 would come out as +0)."""
    return not any(((np.asarray(a, F) == 0) & np.signbit(np.asarray(a, F))).any() for a in arrays)
