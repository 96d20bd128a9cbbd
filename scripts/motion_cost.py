"""Device time of temporal reuse across moving instances (profiles/motion_cost.txt): k_reproject<M2, true> against
k_reproject<M2, false>, and k_gbuffer with and without the INSTANCE output, in one run with time_kernels = 1 on
scenes.moving_instances at the given sizes.

    python scripts/motion_cost.py --sizes 512 1024 --reps 20

Three legs per size and M2 setting: the option off (camera moves; k_reproject<M2, false>), the option on with camera moves only
(k_reproject<M2, true>, every instance STATIC), and the option on with an upload that moves two instances before every camera move
(k_reproject<M2, true>, two of three instances MOVED).
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
    a = ap.parse_args()
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for n in a.sizes:
        steps = [scenes.moving_instances(0), scenes.moving_instances(1)]
        for m2 in (False, True):
            for leg, option, uploads in (("off", 0, False), ("on, static", 1, False), ("on, moved", 1, True)):
                tr = make_hip_tracer(steps[0], n, n, time_kernels=1, object_motion=option)
                rp, gb = [], []
                try:
                    if m2:
                        tr.set_variance()
                    req = ob.make_request(n, n, spp=4, bounces=5)
                    tr.Trace(req, scenes.make_seeds(4, 5))
                    tr.MergeOutput(tr, req)
                    tr.set_temporal()
                    tr.SyncFramebuffer(ob.make_request(n, n, spp=4))
                    for k in ("reproject", "gbuffer"):
                        tr.kernel_ms(k)
                    for r in range(a.reps):
                        sc = steps[(r + 1) % 2]
                        if uploads:
                            tr.UpdateState(0, 1, sc)
                        eye = np.asarray(sc.eye, np.float32) + np.array([0.002 * (r + 1), 0, 0], np.float32)
                        tr.UpdateState(0, 2, dataclasses.replace(sc, eye=eye.astype(np.float32)))
                        tr.SyncFramebuffer(ob.make_request(n, n, spp=4))
                        if uploads and r == 0:
                            continue          # (the first upload's history is the step-0 sync above: as every later one, but discard the warm-up)
                        rp.append(tr.kernel_ms("reproject")[0])
                        gb.append(tr.kernel_ms("gbuffer")[0])
                    symbol = tr.kernel_symbol("reproject")
                    reused = float((tr.read_aov(4)[..., 3] > 0).mean())
                finally:
                    tr.Close()
                print(f"{n}x{n} M2={int(m2)} object_motion {leg:10s}: {symbol:32s} median {med(rp):.4f} ms (min {min(rp):.4f}), "
                      f"k_gbuffer median {med(gb):.4f} ms (min {min(gb):.4f}); history reused on {reused:.3f} of the frame; n {len(rp)}", flush=True)


if __name__ == "__main__":
    main()
