"""The tuning table of DESIGN.md section 10c: variance guidance on the CPU restatements (polaris_host_variance, _denoise_variance,
_reproject_moments) over oracle traces of cornell and cornell-diffuse at 128^2, against a 1024 spp frame.

    python scripts/variance_quality.py > profiles/variance_quality.txt

The per-sample moments come from one-spp oracle traces, trace k fed the seeds of sample k in make_seeds' layout; the accumulator is
their float32 sum in ascending k (rgb | sum L^2), as k_resolve<true> adds them.  Rows: 4 spp, 64 spp, and one camera move (dx = 0.03)
at 1 spp with temporal reuse (TEMPORAL_DEFAULTS; the history is 64 spp at the first view).  RMSE over the filtered pixels, for the
guided filter (DENOISE_DEFAULTS' iterations, normal and depth terms), today's filter (DENOISE_DEFAULTS) and the unfiltered mean."""
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from polaris_amd.hostinfo import size_openmp  # noqa: E402

size_openmp()

import numpy as np  # noqa: E402

import gbuffer_oracle as G  # noqa: E402
import variance_oracle as VO  # noqa: E402
from oracle import pybind as ob  # noqa: E402
from polaris_amd import ctypes_api as T  # noqa: E402
from polaris_amd import host_api, scenes  # noqa: E402

F = np.float32
N = 128
SIGMAS = (1.0, 2.0, 4.0, 8.0)
MIN_SAMPLES = (2, 4, 8)
DN = T.DENOISE_DEFAULTS
TP = T.TEMPORAL_DEFAULTS


def moment_trace(o, sc, spp, base):
    """rgb | sum L^2 of `spp` one-sample traces, sample k fed make_seeds(spp, 5, base)'s seeds of sample k."""
    seeds = scenes.make_seeds(spp, 5, base=base)
    xs = [o.trace(sc, ob.make_request(N, N, spp=1, bounces=5), seeds[k * 6:(k + 1) * 6])[0] for k in range(spp)]
    return VO.moments_of_samples(xs)


def guided(acc, spp, g, a, sigma, ms, temporal=None, prior2=None):
    kw = dict(normal_power_log2=DN["normal_power_log2"], sigma_depth=DN["sigma_depth"], sigma_variance=sigma, min_samples=ms)
    var = host_api.variance(acc, spp, g, a, temporal=temporal, prior2=prior2, **kw)
    c, w = (acc, F(1.0 / float(F(spp)))) if temporal is None else (temporal, F(1))
    return host_api.denoise_variance(c, w, var, g, a, iterations=DN["iterations"], **kw)[..., :3]


def cases(o, name):
    """Yields (label, mask, want, unfiltered, today's filter, guided(sigma, min_samples))."""
    sc0 = scenes.SCENES[name]()
    g0, a0, _ = G.gbuffer(o, sc0, N, N)
    ref, _, _ = o.trace(sc0, ob.make_request(N, N, spp=1024, bounces=5), scenes.make_seeds(1024, 5, base=99))
    for spp, base in ((4, 11), (64, 21)):
        acc = moment_trace(o, sc0, spp, base)
        w = F(1.0 / float(F(spp)))
        yield (f"{spp} spp", G.filtered_mask(a0), ref[..., :3] / 1024, acc[..., :3] * w, host_api.denoise(acc, w, g0, a0, **DN)[..., :3],
               lambda s, m, acc=acc, spp=spp: guided(acc, spp, g0, a0, s, m))
    sc1 = dataclasses.replace(sc0, eye=(np.asarray(sc0.eye, F) + np.array([0.03, 0, 0], F)).astype(F))
    g1, a1, _ = G.gbuffer(o, sc1, N, N)
    ref1, _, _ = o.trace(sc1, ob.make_request(N, N, spp=1024, bounces=5), scenes.make_seeds(1024, 5, base=99))
    acc0 = moment_trace(o, sc0, 64, 7)
    acc1 = moment_trace(o, sc1, 1, 101)
    zero = np.zeros_like(acc0)

    def moved(s, m):
        hist = host_api.temporal_combine(acc0, zero, 0, 64)
        hvar = host_api.variance(acc0, 64, g0, a0, temporal=hist, prior2=zero, normal_power_log2=DN["normal_power_log2"],
                                 sigma_depth=DN["sigma_depth"], sigma_variance=s, min_samples=m)
        prior, prior2 = host_api.reproject_moments(hist, hvar, g0, a0, sc0.eye, sc0.frustum, g1, a1, sc1.eye, sc1.frustum, **TP)
        tmp = host_api.temporal_combine(acc1, prior, 0, 1)
        return guided(acc1, 1, g1, a1, s, m, temporal=tmp, prior2=prior2)

    hist = host_api.temporal_combine(acc0, zero, 0, 64)
    prior = host_api.reproject(hist, g0, a0, sc0.eye, sc0.frustum, g1, a1, sc1.eye, sc1.frustum, **TP)
    tmp = host_api.temporal_combine(acc1, prior, 0, 1)
    yield ("move, 1 spp, temporal", G.filtered_mask(a1), ref1[..., :3] / 1024, tmp[..., :3], host_api.denoise(tmp, F(1), g1, a1, **DN)[..., :3],
           moved)


def main():
    o = ob.Oracle("oracle")
    print(f"{'scene':16s} {'case':22s} {'sigma_v':>7s} {'min_n':>5s} {'guided':>8s} {'atrous':>8s} {'mean':>8s} {'g/atr':>6s} {'g/mean':>6s}")
    for name in ("cornell-diffuse", "cornell"):
        for label, filt, want, raw, old, fn in cases(o, name):
            rmse = lambda x: float(np.sqrt(np.mean((x[filt] - want[filt]) ** 2)))  # noqa: E731
            r_old, r_raw = rmse(old), rmse(raw)
            for s in SIGMAS:
                for m in MIN_SAMPLES:
                    r = rmse(fn(s, m))
                    print(f"{name:16s} {label:22s} {s:7.1f} {m:5d} {r:8.4f} {r_old:8.4f} {r_raw:8.4f} {r / r_old:6.3f} {r / r_raw:6.3f}", flush=True)


if __name__ == "__main__":
    main()
