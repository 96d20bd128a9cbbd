"""What the camera shutter (polaris_hip_set_shutter) costs a frame (profiles/shutter_cost.txt): the headline Cornell frame
(512 x 512, 128 spp, 5 bounces, roulette from bounce 3; tiny-scene mode) and the 58 K-triangle material ball (512 x 512, 32 spp; its
tree does not fit LDS), each traced through the pinhole, the lens, the shutter, and the shutter with the lens.

    python scripts/shutter_cost.py [--reps 9]

Per scene and setting: the median wall time of a Trace over --reps frames on a tracer WITHOUT kernel timers, then on a second tracer
with time_kernels = 1 the per-frame sums of the timers "generate", "intersect" and "intersect_packet" (median over the same number of
frames) with the kernel symbol each timer bracketed.  The lens is scripts/lens_cost.py's (round, 0.02 x the scene's extent, focused on
the middle of the scene); the shutter closes at the eye moved 0.05 x the extent along TR - TL with the frustum turned 2 degrees about
the up vector, focused 1.25 x further (the cameras of tests/test_gpu_shutter.py).  No target is set: the shutter's plan is the lens'
(per-ray origins, no shared-origin traversal variants), its generator blends 19 (lens: 29) floats per ray, and its rays are a little
less coherent than one eye's; the file records what that is.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

TIMERS = ("generate", "intersect", "intersect_packet")
SETTINGS = (("pinhole", False, False), ("lens", True, False), ("shutter", False, True), ("shutter + lens", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter_cost.txt"))
    a = ap.parse_args()

    from conftest import make_hip_tracer
    from lens_cost import lens_of
    from oracle import pybind as ob
    from polaris_amd import scenes
    from shutter_oracle import close_camera

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = []
    for name, make, W, H, spp in (("cornell_box (headline)", scenes.cornell_box, 512, 512, 128), ("material_ball", scenes.material_ball, 512, 512, 32)):
        sc = make()
        B, rr = 5, 3
        seeds = scenes.make_seeds(spp, B)
        radius, focus = lens_of(sc)
        eye1, frustum1 = close_camera(sc)
        for label, lens, shutter in SETTINGS:
            walls, sums, symbols = [], {t: [] for t in TIMERS}, {}
            for timed in (False, True):
                tr = make_hip_tracer(sc, W, H, time_kernels=1 if timed else 0)
                try:
                    if lens:
                        tr.set_lens(radius, focus)
                    if shutter:
                        tr.set_shutter(eye1, frustum1, 1.25 * focus if lens else None)
                    for _ in range(2):                                   # warm-up: allocations, first launches
                        tr.Trace(ob.make_request(W, H, spp=spp, bounces=B, rr=rr), seeds)
                    for t in TIMERS:
                        tr.kernel_ms(t)                                  # (reading a timer resets it)
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        tr.Trace(ob.make_request(W, H, spp=spp, bounces=B, rr=rr), seeds)
                        if not timed:
                            walls.append((time.perf_counter() - t0) * 1e3)
                        else:
                            for t in TIMERS:
                                sums[t].append(tr.kernel_ms(t)[0])
                                symbols[t] = tr.kernel_symbol(t) if sums[t][-1] > 0 else "-"
                finally:
                    tr.Close()
            timers = ", ".join(f"{t} {med(sums[t]):.3f} ms [{symbols[t]}]" for t in TIMERS)
            lines.append(f"{name}, {sc.num_triangles} triangles, {W}x{H} @ {spp} spp, {label:14s}: frame median {med(walls):.3f} ms "
                         f"(min {min(walls):.3f}, n {a.reps}); {timers}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
