"""Device time of temporal reuse across mesh deformation (profiles/vertex_motion_cost.txt): k_reproject_deform<M2> against
k_reproject<M2, true>, and k_gbuffer with and without the HIT output, in one run with time_kernels = 1 on the two-instance Cornell
box of tests/vertex_motion_oracle.py at the given sizes.

    python scripts/vertex_motion_cost.py --sizes 512 1024 --reps 20

Three legs per size and M2 setting, all with "object_motion" and "vertex_update" on: the option off with camera moves
(k_reproject<M2, true>, k_gbuffer without HIT), the option on with camera moves only (k_reproject<M2, true>: the history has no
snapshot; k_gbuffer with HIT), and the option on with an update_vertices that deforms the tall block before every camera move
(k_reproject_deform<M2>).
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
    import vertex_motion_oracle as VO
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    base = VO.cornell_two_instances()
    steps = [VO.deformed_block(base, 1), VO.deformed_block(base, 2)]
    updates = [scenes.vertex_update_args(s) for s in steps]
    for n in a.sizes:
        for m2 in (False, True):
            for leg, option, deforms in (("off", 0, False), ("on, camera", 1, False), ("on, deformed", 1, True)):
                tr = make_hip_tracer(base, n, n, time_kernels=1, object_motion=1, vertex_update=1, vertex_motion=option)
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
                        if deforms:
                            v, boxes, _, _, ems = updates[r % 2]
                            tr.update_vertices(v, boxes, None, None, ems)
                        eye = np.asarray(base.eye, np.float32) + np.array([0.002 * (r + 1), 0, 0], np.float32)
                        tr.UpdateState(0, 2, dataclasses.replace(base, eye=eye.astype(np.float32)))
                        tr.SyncFramebuffer(ob.make_request(n, n, spp=4))
                        rp.append(tr.kernel_ms("reproject")[0])
                        gb.append(tr.kernel_ms("gbuffer")[0])
                    symbol = tr.kernel_symbol("reproject")
                    reused = float((tr.read_aov(4)[..., 3] > 0).mean())
                finally:
                    tr.Close()
                print(f"{n}x{n} M2={int(m2)} vertex_motion {leg:12s}: {symbol:32s} median {med(rp):.4f} ms (min {min(rp):.4f}), "
                      f"k_gbuffer median {med(gb):.4f} ms (min {min(gb):.4f}); history reused on {reused:.3f} of the frame; n {len(rp)}", flush=True)


if __name__ == "__main__":
    main()
