"""Device time of the denoiser per denoised sync (profiles/denoise_cost.txt): the G-buffer pass and the K filter iterations,
with time_kernels = 1, on the headline scene at the given sizes.

    python scripts/denoise_cost.py --sizes 512 1024 --iterations 5 --reps 20
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="cornell")
    a = ap.parse_args()
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes

    for n in a.sizes:
        sc = scenes.SCENES[a.scene]()
        tr = make_hip_tracer(sc, n, n, time_kernels=1)
        try:
            req = ob.make_request(n, n, spp=4, bounces=5)
            tr.Trace(req, scenes.make_seeds(4, 5))
            tr.MergeOutput(tr, req)
            tr.set_denoise(iterations=a.iterations)
            for k in ("gbuffer", "denoise", "tonemap"):
                tr.kernel_ms(k)
            gb = []
            dn = []
            tm = []
            for _ in range(a.reps):
                tr.UpdateState(0, 2, sc)  # set_camera: the next sync recomputes the G-buffer
                tr.SyncFramebuffer(ob.make_request(n, n, spp=4))
                gb.append(tr.kernel_ms("gbuffer")[0])
                dn.append(tr.kernel_ms("denoise")[0])
                tm.append(tr.kernel_ms("tonemap")[0])
        finally:
            tr.Close()
        px = n * n
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        # algorithmic bytes: G-buffer = 32 B/px written (+ the traversal's and material walk's reads, scene-dependent);
        # filter iteration = frame acc or r^k 16 + guide 16 + albedo 16 read, 16 written per pixel (taps beyond the centre hit caches)
        print(f"{a.scene} {n}x{n} K={a.iterations}: gbuffer {med(gb):.4f} ms (min {min(gb):.4f}), denoise {med(dn):.4f} ms "
              f"(min {min(dn):.4f}; {med(dn) / a.iterations:.4f} ms per iteration), tonemap {med(tm):.4f} ms; "
              f"filter {64 * px * a.iterations / 1e6:.1f} MB algorithmic ({64 * px * a.iterations / (med(dn) * 1e-3) / 1e9:.0f} GB/s), "
              f"G-buffer writes {32 * px / 1e6:.1f} MB; medians of {a.reps}")


if __name__ == "__main__":
    main()
