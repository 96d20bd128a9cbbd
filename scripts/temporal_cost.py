"""Device time of temporal reuse (profiles/temporal_cost.txt): k_reproject once per camera move and k_temporal per sync, with
time_kernels = 1, on the headline scene at the given sizes.

    python scripts/temporal_cost.py --sizes 512 1024 --reps 20
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="cornell")
    a = ap.parse_args()
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes

    for n in a.sizes:
        sc = scenes.SCENES[a.scene]()
        tr = make_hip_tracer(sc, n, n, time_kernels=1)
        rp, tp = [], []
        try:
            req = ob.make_request(n, n, spp=4, bounces=5)
            tr.Trace(req, scenes.make_seeds(4, 5))
            tr.MergeOutput(tr, req)
            tr.set_temporal()
            tr.SyncFramebuffer(ob.make_request(n, n, spp=4))
            for k in ("reproject", "temporal"):
                tr.kernel_ms(k)
            for r in range(a.reps):
                # a move (the corners are eye-relative: a sideways shift keeps them), then one sync: one k_reproject, one k_temporal
                eye = np.asarray(sc.eye, np.float32) + np.array([0.002 * (r + 1), 0, 0], np.float32)
                tr.UpdateState(0, 2, dataclasses.replace(sc, eye=eye.astype(np.float32)))
                tr.SyncFramebuffer(ob.make_request(n, n, spp=4))
                rp.append(tr.kernel_ms("reproject")[0])
                tp.append(tr.kernel_ms("temporal")[0])
            reused = float((tr.read_aov(4)[..., 3] > 0).mean())
        finally:
            tr.Close()
        px = n * n
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        # algorithmic bytes: reproject = guide 16 + albedo 16 + 4 taps x (history 16 + guide 16 + albedo 16) read, 16 written per
        # pixel; temporal = accumulator 16 + prior 16 read, 16 written
        print(f"{a.scene} {n}x{n}: reproject {med(rp):.4f} ms (min {min(rp):.4f}; {240 * px / (med(rp) * 1e-3) / 1e9:.0f} GB/s "
              f"algorithmic), temporal {med(tp):.4f} ms (min {min(tp):.4f}; {48 * px / (med(tp) * 1e-3) / 1e9:.0f} GB/s); "
              f"history reused on {reused:.3f} of the frame; medians of {a.reps}", flush=True)


if __name__ == "__main__":
    main()
