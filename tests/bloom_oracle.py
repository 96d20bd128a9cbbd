"""An independent numpy statement of the bloom of the display stage, written from DESIGN.md section 10m's text: the levels, the bright
pass, the {1, 3, 3, 1} / 8 downsample (with the Karis weighting of level 1), the 2 x tent upsample and the bloomed byte.  Every
operation is float32 in the order the section gives, so the result is meant to equal polaris_host_bloom (polaris_amd/host/bloom.cpp)
bit for bit; it shares no code with polaris_amd/csrc/bloom.h.  Whole levels are computed at once by gathering with clamped index
arrays.  dtype = np.float64 evaluates the same pyramid in double (the conservation test's reference).  The exposure, the tone
operators and the transfer functions are display_oracle's.
"""
import numpy as np

import display_oracle as DO

F = np.float32
K = (0.125, 0.375, 0.375, 0.125)


def level_sizes(W, rows, levels):
    """[(w_0, h_0), (w_1, h_1), ... (w_L, h_L)]: halved rounding up; L = min(levels, the first level of one pixel), at least 1."""
    sizes = [(W, rows)]
    for l in range(1, levels + 1):
        w, h = sizes[-1]
        sizes.append(((w + 1) // 2, (h + 1) // 2))
        if sizes[-1] == (1, 1):
            break
    return sizes


def bright(rgb, weight, exposure, E, threshold, knee, dtype=F):
    """b of (h, w, 3) source pixels."""
    T = dtype
    with np.errstate(all="ignore"):
        c = ((np.asarray(rgb, F)[..., :3] * F(weight)) * F(exposure)) * F(E)     # the displayed value is float32 in either mode
        c = np.where(c > 0, np.minimum(c, F(65536.0)), F(0.0)).astype(T)        # NaN and <= 0: 0
    m = np.maximum(np.maximum(c[..., 0], c[..., 1]), c[..., 2])
    k = T(threshold) * T(knee)
    s = np.minimum(np.maximum((m - T(threshold)) + k, T(0.0)), T(2.0) * k)
    s = (s * s) / (T(4.0) * k + T(1e-5))
    f = np.maximum(s, m - T(threshold)) / np.maximum(m, T(1e-5))
    return (c * f[..., None]).astype(T)


def down(src, karis=False, dtype=F):
    """D of the next level from (h, w, 3) src; karis: the taps weighted by 1 / (1 + luminance)."""
    T = dtype
    h, w = src.shape[:2]
    dw, dh = (w + 1) // 2, (h + 1) // 2
    xs, ys = 2 * np.arange(dw) - 1, 2 * np.arange(dh) - 1
    if karis:
        wt = T(1.0) / (T(1.0) + ((T(F(0.2126)) * src[..., 0] + T(F(0.7152)) * src[..., 1]) + T(F(0.0722)) * src[..., 2]))
    acc, accw = np.zeros((dh, dw, 3), T), np.zeros((dh, dw), T)
    for j in range(4):
        yy = np.clip(ys + j, 0, h - 1)[:, None]
        row, roww = np.zeros((dh, dw, 3), T), np.zeros((dh, dw), T)
        for i in range(4):
            xx = np.clip(xs + i, 0, w - 1)[None, :]
            t = src[yy, xx]
            if karis:
                row = row + T(K[i]) * (t * wt[yy, xx][..., None])
                roww = roww + T(K[i]) * wt[yy, xx]
            else:
                row = row + T(K[i]) * t
        acc = acc + T(K[j]) * row
        accw = accw + T(K[j]) * roww
    return (acc / accw[..., None] if karis else acc).astype(T)


def _tent(n_fine, n_coarse, dtype):
    i = np.arange(n_fine)
    odd = (i & 1) == 1
    a = np.where(odd, i >> 1, (i >> 1) - 1)
    wa = np.where(odd, dtype(0.75), dtype(0.25)).astype(dtype)
    return np.clip(a, 0, n_coarse - 1), np.clip(a + 1, 0, n_coarse - 1), wa, (dtype(1.0) - wa).astype(dtype)


def up(U, w, h, dtype=F):
    """up(U) at the (h, w) pixels of the finer level: x inside y."""
    ch, cw = U.shape[:2]
    xa, xb, wxa, wxb = _tent(w, cw, dtype)
    ya, yb, wya, wyb = _tent(h, ch, dtype)
    wxa, wxb, wya, wyb = wxa[None, :, None], wxb[None, :, None], wya[:, None, None], wyb[:, None, None]
    top = wxa * U[ya[:, None], xa[None, :]] + wxb * U[ya[:, None], xb[None, :]]
    bottom = wxa * U[yb[:, None], xa[None, :]] + wxb * U[yb[:, None], xb[None, :]]
    return (wya * top + wyb * bottom).astype(dtype)


def pyramid(rgb, *, weight=1.0, exposure=1.0, E=1.0, levels=5, threshold=1.0, knee=0.5, karis=1, dtype=F):
    """(D_1 .. D_L, U_1, the full-resolution term up(U_1) / L, L) over the (h, w, 3+) region."""
    h, w = rgb.shape[:2]
    sizes = level_sizes(w, h, levels)
    L = len(sizes) - 1
    D = [down(bright(rgb, weight, exposure, E, threshold, knee, dtype), bool(karis), dtype)]
    for l in range(2, L + 1):
        D.append(down(D[-1], False, dtype))
    assert [d.shape[:2] for d in D] == [(hh, ww) for ww, hh in sizes[1:]]
    U = D[-1]
    for l in range(L - 1, 0, -1):
        U = (D[l - 1] + up(U, sizes[l][0], sizes[l][1], dtype)).astype(dtype)
    term = (up(U, w, h, dtype) / dtype(L)).astype(dtype)
    return D, U, term, L


def bloom(plane, *, weight=1.0, exposure=1.0, block_y=0, block_h=None, rgba=None, prev_log2E=None, display=None, levels=5, threshold=1.0, knee=0.5,
          intensity=0.25, karis=1):
    """A bloomed displayed sync over the request's rows of an (H, W, 4) plane: (RGBA8, U_1 | 0, the term | 0, levels used)."""
    d = dict(tone_operator=DO.REINHARD, srgb=0, white=4.0, auto_exposure=0)
    d.update(display or {})
    plane = np.asarray(plane, F)
    H, W = plane.shape[:2]
    rows = slice(block_y, H if block_h is None else block_y + block_h)
    fb, _, info = DO.display(plane, weight=weight, exposure=exposure, block_y=block_y, block_h=block_h, rgba=rgba, prev_log2E=prev_log2E, **d)
    E = info["E"] if d["auto_exposure"] else F(1)
    src = plane[rows, :, :3]
    _, U1, term, L = pyramid(src, weight=weight, exposure=exposure, E=E, levels=levels, threshold=threshold, knee=knee, karis=karis)
    with np.errstate(all="ignore"):
        c = ((src * F(weight)) * F(exposure)) * F(E) + F(intensity) * term
        t = DO.transfer(DO.tone(c, d["tone_operator"], d["white"]), d["srgb"])
        v = np.minimum(np.maximum(t, F(0.0)), F(1.0)) * F(255.0)
        fb[rows, :, :3] = np.where(np.isnan(v), 0, v).astype(np.uint8)
    fb[rows, :, 3] = 255

    def four(a):
        return np.concatenate([a, np.zeros(a.shape[:2] + (1,), F)], axis=2)
    return fb, four(U1), four(term), L
