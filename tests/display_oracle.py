"""An independent numpy statement of the display stage, written from DESIGN.md section 10l's text: the luminance histogram, the
exposure it implies, the four tone operators, the two transfer functions and the byte.  Every operation is float32 in the order the
section gives, so the result is meant to equal polaris_host_display (polaris_amd/host/display.cpp) bit for bit; it shares no code
with polaris_amd/csrc/display.h.  pm_log / pm_exp / pm_pow restate include/polaris_math.h (Cephes logf / expf) on arrays.
"""
import numpy as np

F = np.float32
REINHARD, REINHARD_WHITE, ACES, HABLE = 0, 1, 2, 3
BINS = 256


def _f(x):
    return np.asarray(x, dtype=F)


def pm_log(x):
    """include/polaris_math.h pm_log for x > 0 finite, elementwise in float32."""
    x = _f(x).copy()
    e = np.zeros(x.shape, np.int32)
    small = x < F(1.17549435e-38)
    x[small] = x[small] * F(16777216.0)
    e[small] = -24
    u = x.view(np.uint32)
    e = e + ((u >> 23) & 0xFF).astype(np.int32) - 126
    m = ((u & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(F)
    low = m < F(0.707106781186547524)
    e = np.where(low, e - 1, e)
    m = np.where(low, (m + m) - F(1.0), m - F(1.0)).astype(F)
    z = m * m
    y = F(7.0376836292e-2) * m - F(1.1514610310e-1)
    for c, sign in ((1.1676998740e-1, 1), (1.2420140846e-1, -1), (1.4249322787e-1, 1), (1.6668057665e-1, -1), (2.0000714765e-1, 1),
                    (2.4999993993e-1, -1), (3.3333331174e-1, 1)):
        y = y * m + F(c) if sign > 0 else y * m - F(c)
    y = (y * m) * z
    fe = e.astype(F)
    y = y + F(-2.12194440e-4) * fe
    y = y + F(-0.5) * z
    z = m + y
    return (z + F(0.693359375) * fe).astype(F)


def pm_exp(x):
    """include/polaris_math.h pm_exp, elementwise in float32."""
    x = _f(x).copy()
    big, tiny = x > F(88.72283905206835), x < F(-87.0)
    x = np.where(big | tiny | np.isnan(x), F(0.0), x).astype(F)
    fn = np.floor(F(1.44269504088896341) * x + F(0.5)).astype(F)
    n = fn.astype(np.int32)
    x = x - fn * F(0.693359375)
    x = x - fn * F(-2.12194440e-4)
    z = x * x
    p = F(1.9875691500e-4) * x + F(1.3981999507e-3)
    for c in (8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = p * x + F(c)
    z = ((p * z) + x) + F(1.0)
    over = n > 127
    z = np.where(over, z * F(2.0), z).astype(F)
    n = np.where(over, n - 1, n)
    out = (z * ((n + 127).astype(np.uint32) << 23).view(F)).astype(F)
    out = np.where(big, F(3.402823466e+38), out)
    return np.where(tiny, F(0.0), out).astype(F)


def pm_pow(x, y):
    """include/polaris_math.h pm_pow: x > 0: pm_exp(y pm_log(x)); x = 0: 0; negative or NaN: NaN."""
    x = _f(x)
    pos = x > 0
    r = pm_exp(F(y) * pm_log(np.where(pos, x, F(1.0))))
    return np.where(pos, r, np.where(x == 0, F(0.0), F(np.nan))).astype(F)


def luminance(rgb, weight):
    """L = (0.2126 r + 0.7152 g) + 0.0722 b of rgb * weight."""
    with np.errstate(all="ignore"):
        c = _f(rgb) * F(weight)
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def bins_of(L):
    """The bin of every luminance, -1 = not metered: finite and >= 2^-16; 8 (e + 16) + the top three mantissa bits; >= 2^16 in 255."""
    L = _f(L)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(L) & (L >= F(2.0 ** -16))
    u = np.where(ok, L, F(1.0)).view(np.uint32).astype(np.int64)
    e = (u >> 23) - 127
    k = (u >> 20) & 7
    return np.where(ok, np.minimum(8 * (e + 16) + k, BINS - 1), -1)


def histogram(rgb, weight):
    b = bins_of(luminance(rgb, weight)).ravel()
    return np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32)


def bin_values():
    """e + log2(1 + (k + 1/2) / 8) in double, rounded to float32."""
    b = np.arange(BINS)
    return ((b // 8 - 16).astype(np.float64) + np.log2(1.0 + ((b % 8) + 0.5) / 8.0)).astype(F)


def expose(counts, *, key, compensation_ev, low_permille, high_permille, min_ev, max_ev, adapt, prev_log2E=None):
    """The exposure info of one sync from its 256 counts and the state it starts from (prev_log2E = None: none)."""
    counts = [int(c) for c in counts]
    N = sum(counts)
    if N == 0:
        if prev_log2E is None:
            return {"valid": 0, "n_metered": 0, "avg": F(0), "log2E": F(0), "E": F(1)}
        return {"valid": 1, "n_metered": 0, "avg": F(0), "log2E": F(prev_log2E), "E": pm_exp(F(prev_log2E) * F(0.69314718055994530942))[()]}
    lo = N * int(low_permille) // 1000
    hi = max(N * int(high_permille) // 1000, lo + 1)
    value = bin_values()
    total, cum = F(0), 0
    for b in range(BINS):
        n = min(cum + counts[b], hi) - max(cum, lo)
        if n > 0:
            total = F(total + F(n) * value[b])
        cum += counts[b]
    avg = F(total / F(hi - lo))
    log2_key = F(np.log2(np.float64(F(key))))
    target = F(F(log2_key - avg) + F(compensation_ev))
    target = min(max(target, F(min_ev)), F(max_ev))
    log2E = target if prev_log2E is None else F(F(prev_log2E) + F(F(target - F(prev_log2E)) * F(adapt)))
    return {"valid": 1, "n_metered": N, "avg": avg, "log2E": F(log2E), "E": pm_exp(F(log2E) * F(0.69314718055994530942))[()]}


def hable(x):
    x = _f(x)
    return (x * (F(0.15) * x + F(0.05)) + F(0.004)) / (x * (F(0.15) * x + F(0.50)) + F(0.06)) - F(0.02) / F(0.30)


def tone(c, op, white):
    c = _f(c)
    with np.errstate(all="ignore"):
        if op == REINHARD:
            return c / (c + F(1.0))
        if op == REINHARD_WHITE:
            return (c * (F(1.0) + c / (F(white) * F(white)))) / (F(1.0) + c)
        if op == ACES:
            return (c * (F(2.51) * c + F(0.03))) / (c * (F(2.43) * c + F(0.59)) + F(0.14))
        return hable(c) / hable(F(white))


def transfer(m, srgb):
    m = _f(m)
    with np.errstate(all="ignore"):
        if not srgb:
            return pm_pow(m, F(1.0) / F(2.2))
        return np.where(m <= F(0.0031308), F(12.92) * m, F(1.055) * pm_pow(m, F(1.0) / F(2.4)) - F(0.055)).astype(F)


def to_bytes(rgb, weight, exposure, E, *, op, srgb, white):
    """(…, 4) uint8 of (…, 3+) float32: c = ((rgb weight) exposure) E per channel, tone, transfer, clamp, times 255, truncated; NaN: 0."""
    with np.errstate(all="ignore"):
        c = ((_f(rgb)[..., :3] * F(weight)) * F(exposure)) * F(E)
        t = transfer(tone(c, op, white), srgb)
        v = np.minimum(np.maximum(t, F(0.0)), F(1.0)) * F(255.0)        # (np.maximum / np.minimum pass a NaN on)
        out = np.zeros(c.shape[:-1] + (4,), np.uint8)
        out[..., :3] = np.where(np.isnan(v), 0, v).astype(np.uint8)
    out[..., 3] = 255
    return out


def display(plane, *, weight=1.0, exposure=1.0, block_y=0, block_h=None, rgba=None, prev_log2E=None, tone_operator=REINHARD, srgb=0, white=4.0,
            auto_exposure=0, key=0.18, compensation_ev=0.0, low_permille=500, high_permille=950, min_ev=-16.0, max_ev=16.0, adapt=1.0):
    """The whole stage over the request's rows of an (H, W, 4) plane: (RGBA8, the 256 counts, the exposure info)."""
    plane = _f(plane)
    H, W = plane.shape[:2]
    rows = slice(block_y, H if block_h is None else block_y + block_h)
    fb = np.zeros((H, W, 4), np.uint8) if rgba is None else np.array(rgba, np.uint8, copy=True)
    counts = np.zeros(BINS, np.uint32)
    info = {"valid": 0 if prev_log2E is None else 1, "n_metered": 0, "avg": F(0), "log2E": F(0 if prev_log2E is None else prev_log2E), "E": F(1)}
    if auto_exposure:
        counts = histogram(plane[rows, :, :3], weight)
        info = expose(counts, key=key, compensation_ev=compensation_ev, low_permille=low_permille, high_permille=high_permille, min_ev=min_ev,
                      max_ev=max_ev, adapt=adapt, prev_log2E=prev_log2E)
    fb[rows] = to_bytes(plane[rows], weight, exposure, info["E"] if auto_exposure else F(1), op=tone_operator, srgb=srgb, white=white)
    return fb, counts, info
