"""Device time of variance guidance (profiles/variance_cost.txt), time_kernels = 1, on the headline scene: the batch epilogue with
and without the moments (k_resolve<true> / k_resolve<false>), k_variance per sync and one variance-guided a-trous iteration
(k_denoise_variance) against today's (k_denoise), at the given sizes.

k_variance is timed on both of its paths: the per-pixel estimate (16 spp >= min_samples 8) and the 7 x 7 spatial fallback (4 spp at
the default min_samples 8, every filtered pixel below it), and with temporal reuse after a camera move at 1 spp, at the defaults
(n_eff = 1 + m: per-pixel where the history holds, spatial where it does not) and with min_samples 64 (every pixel spatial, with the
TEMPORAL and PRIOR2 loads of each tap).

    python scripts/variance_cost.py --sizes 512 1024 --reps 20
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TIMERS = ("resolve", "variance", "denoise", "denoise_variance")


def med(v):
    return sorted(v)[len(v) // 2] if v else float("nan")


def run(n, scene, spp, reps, *, variance=True, min_samples=None, temporal=False):
    """Medians (ms) of each timer over `reps` frames (resolve: per launch).  temporal: every frame is a camera move followed by
    one Trace + sync, so each sync reprojects a history of the previous view."""
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes

    sc = scenes.SCENES[scene]()
    tr = make_hip_tracer(sc, n, n, time_kernels=1)
    t = {k: [] for k in TIMERS}
    spatial = float("nan")
    try:
        tr.set_denoise(**{**T.DENOISE_DEFAULTS, "iterations": 1})
        if temporal:
            tr.set_temporal(**T.TEMPORAL_DEFAULTS)
        if variance:
            tr.set_variance(**{**T.VARIANCE_DEFAULTS, **({} if min_samples is None else {"min_samples": min_samples})})
        req = ob.make_request(n, n, spp=spp, bounces=5)
        for r in range(reps + 2):
            if temporal and r:
                eye = np.asarray(sc.eye, np.float32) + np.array([0.002 * r, 0, 0], np.float32)
                tr.UpdateState(0, 2, dataclasses.replace(sc, eye=eye.astype(np.float32)))
            for k in TIMERS:
                tr.kernel_ms(k)
            tr.Trace(req, scenes.make_seeds(spp, 5, base=r))
            tr.MergeOutput(tr, req)
            tr.SyncFramebuffer(ob.make_request(n, n, spp=spp))
            ms = {k: tr.kernel_ms(k) for k in TIMERS}
            if r >= 2:   # (the first frames allocate, and under temporal reuse the first has no history)
                for k, (v, launches) in ms.items():
                    if launches:
                        t[k].append(v / launches if k == "resolve" else v)
        if variance:
            import gbuffer_oracle as G

            var = tr.read_aov(T.AOV_VARIANCE)
            filt = G.filtered_mask(tr.read_aov(T.AOV_ALBEDO))
            ms_eff = T.VARIANCE_DEFAULTS["min_samples"] if min_samples is None else min_samples
            spatial = float(((var[..., 2] < max(ms_eff, 2)) & filt).sum() / max(filt.sum(), 1))
    finally:
        tr.Close()
    return {k: med(v) for k, v in t.items()}, {k: (min(v) if v else float("nan")) for k, v in t.items()}, spatial


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="cornell")
    a = ap.parse_args()
    for n in a.sizes:
        off, _, _ = run(n, a.scene, 16, a.reps, variance=False)
        on, on_min, _ = run(n, a.scene, 16, a.reps)
        print(f"{a.scene} {n}x{n} 16 spp: resolve per launch {off['resolve']:.4f} ms -> moments {on['resolve']:.4f} ms; one a-trous "
              f"iteration {off['denoise']:.4f} ms -> guided {on['denoise_variance']:.4f} ms (min {on_min['denoise_variance']:.4f})", flush=True)
        for label, kw in (("16 spp, per-pixel", dict(spp=16)), ("4 spp, spatial", dict(spp=4)),
                          ("temporal, move, 1 spp", dict(spp=1, temporal=True)),
                          ("temporal, move, 1 spp, min_samples 64", dict(spp=1, temporal=True, min_samples=64))):
            m, mn, spatial = run(n, a.scene, kw.pop("spp"), a.reps, **kw)
            print(f"{a.scene} {n}x{n} {label}: k_variance {m['variance']:.4f} ms (min {mn['variance']:.4f}), spatial fallback on "
                  f"{spatial:.3f} of the filtered pixels; guided iteration {m['denoise_variance']:.4f} ms; medians of {a.reps}", flush=True)


if __name__ == "__main__":
    main()
