"""The tuning table of DESIGN.md section 10b: temporal reuse on the CPU restatements (polaris_host_reproject, _temporal_combine,
_denoise) over oracle traces of cornell and cornell-diffuse at 128^2, against a 1024 spp frame at the last view.

    python scripts/temporal_quality.py > profiles/temporal_quality.txt

Rows: one move by dx = 0.03 (about 3 pixels of parallax on the back wall) at 1 spp, a chain of 8 moves by 0.01 at 1 spp each, and
one move at 64 spp; the history starts as 64 spp at the first view.  RMSE over the filtered pixels of the last view (misses and
emitters pass through both pipelines as the same acc * weight), with and without the a-trous filter (DENOISE_DEFAULTS)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from polaris_amd.hostinfo import size_openmp  # noqa: E402

size_openmp()

import dataclasses  # noqa: E402

import numpy as np  # noqa: E402

import gbuffer_oracle as G  # noqa: E402
from oracle import pybind as ob  # noqa: E402
from polaris_amd import ctypes_api as T  # noqa: E402
from polaris_amd import host_api, scenes  # noqa: E402

F = np.float32
N = 128
CASES = [("one move, 1 spp", 0.03, 1, 1), ("8 moves, 1 spp", 0.01, 1, 8), ("one move, 64 spp", 0.03, 64, 1)]
PARAMS = [dict(max_history=m, normal_threshold=nt, depth_threshold=dt) for m, nt, dt in
          [(4, 0.9, 0.1), (16, 0.9, 0.1), (32, 0.9, 0.1), (64, 0.9, 0.1), (16, 0.8, 0.1), (16, 0.95, 0.1), (16, 0.9, 0.05), (16, 0.9, 0.2)]]


def main():
    o = ob.Oracle("oracle")
    print(f"{'scene':16s} {'case':18s} {'max_h':>5s} {'n_thr':>5s} {'d_thr':>5s} {'reused':>6s} {'tmp+atr':>8s} {'atrous':>8s} {'ratio':>6s} "
          f"{'tmp raw':>8s} {'raw':>8s} {'ratio':>6s}")
    for name in ("cornell-diffuse", "cornell"):
        sc0 = scenes.SCENES[name]()
        cache = {}

        def trace(dx, spp, base):
            key = (round(dx, 6), spp, base)
            if key not in cache:
                sc = dataclasses.replace(sc0, eye=(np.asarray(sc0.eye, F) + np.array([dx, 0, 0], F)).astype(F))
                acc, _, _ = o.trace(sc, ob.make_request(N, N, spp=spp, bounces=5), scenes.make_seeds(spp, 5, base=base))
                g, a, _ = G.gbuffer(o, sc, N, N)
                cache[key] = (sc, acc, g, a)
            return cache[key]

        for label, dx, spp, steps in CASES:
            _, ref, _, _ = trace(dx * steps, 1024, 99)
            want = ref[..., :3] / 1024
            for p in PARAMS:
                sc, acc0, g0, a0 = trace(0.0, 64, 7)
                hist = host_api.temporal_combine(acc0, np.zeros_like(acc0), 0, 64)
                for k in range(1, steps + 1):
                    sck, acc, g, a = trace(dx * k, spp, 100 + k)
                    prior = host_api.reproject(hist, g0, a0, sc.eye, sc.frustum, g, a, sck.eye, sck.frustum, **p)
                    hist = host_api.temporal_combine(acc, prior, 0, spp)
                    sc, g0, a0 = sck, g, a
                filt = G.filtered_mask(a0)
                rmse = lambda x: float(np.sqrt(np.mean((x[filt] - want[filt]) ** 2)))  # noqa: E731
                tmp = host_api.denoise(hist, F(1), g0, a0, **T.DENOISE_DEFAULTS)[..., :3]
                spatial = host_api.denoise(acc, F(1.0 / F(spp)), g0, a0, **T.DENOISE_DEFAULTS)[..., :3]
                t, s, tr, r = rmse(tmp), rmse(spatial), rmse(hist[..., :3]), rmse(acc[..., :3] / spp)
                print(f"{name:16s} {label:18s} {p['max_history']:5d} {p['normal_threshold']:5.2f} {p['depth_threshold']:5.2f} "
                      f"{(prior[filt, 3] > 0).mean():6.3f} {t:8.4f} {s:8.4f} {t / s:6.3f} {tr:8.4f} {r:8.4f} {tr / r:6.3f}", flush=True)


if __name__ == "__main__":
    main()
