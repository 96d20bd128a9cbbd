"""What a camera projection (polaris_hip_set_projection) costs a frame (profiles/projection_cost.txt): the headline Cornell
frame (512 x 512, 128 spp, 5 bounces, roulette from bounce 3; tiny-scene mode) and the 58 K-triangle material ball (512 x 512, 32 spp;
its tree does not fit LDS), each traced through the perspective camera, the orthographic one and the equirectangular one.

    python scripts/projection_cost.py [--reps 9]

Per scene and setting: the median wall time of a Trace over --reps frames on a tracer WITHOUT kernel timers, then on a second tracer
with time_kernels = 1 the per-frame sums of the timers "generate", "intersect" and "intersect_packet" (median over the same number of
frames) with the kernel symbol each timer bracketed.  The orthographic window is as high as the scene's extent; the panorama spans
120 x 60 degrees, so that the scene fills the frame as it does the perspective one (a full panorama from outside the scene is mostly
sky, which is cheap and says nothing).  Both look along the frustum's basis (tests/projection_oracle.py scene_projection).  No
target is set: the projection's plan is the lens' (per-ray origins, no shared-origin traversal variants) and the equirectangular
generator also pays four pm_sin / pm_cos per ray; the file records what that is.  The images differ, so the frames are not the same
work: the "intersect" column says how much of a difference is the rays' and how much the generator's.

The last lines are the compiler's figures of the new kernels (VGPRs, scratch bytes, waves per SIMD), filled in by hand from
scripts/isa_stats.py's listing of the library's device code.
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
SETTINGS = (("perspective", 0), ("orthographic", 1), ("equirect 120x60", 2))
KERNELS = """compiler (hipcc --offload-arch=gfx950, the library's flags): VGPRs | scratch bytes | waves per SIMD (512 VGPRs, 8 at most)
  k_generate_proj<1> 10 | 0 | 8      k_generate_proj<2> 18 | 0 | 8      (k_generate 14, k_generate_lens 17, k_generate_shutter 24 / 28: unchanged)
  k_gbuffer_proj 81 | 0 | 5          k_gbuffer_chain_proj 90 | 0 | 5    (k_gbuffer 81, k_gbuffer_chain 90: unchanged; the 32 KB LDS stack allows 5 too)
  k_reproject_proj<M2, MOTION> 29 / 32 / 33 / 32 | 0 | 8               (k_reproject 29 / 33 / 33 / 34: unchanged)
  k_reproject_deform_proj<M2> 48 / 50 | 0 | 8                           (k_reproject_deform 42 / 46: unchanged)"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_cost.txt"))
    a = ap.parse_args()

    import numpy as np

    import projection_oracle as PO
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = []
    for name, make, W, H, spp in (("cornell_box (headline)", scenes.cornell_box, 512, 512, 128), ("material_ball", scenes.material_ball, 512, 512, 32)):
        sc = make()
        B, rr = 5, 3
        seeds = scenes.make_seeds(spp, B)
        for label, kind in SETTINGS:
            walls, sums, symbols = [], {t: [] for t in TIMERS}, {}
            for timed in (False, True):
                tr = make_hip_tracer(sc, W, H, time_kernels=1 if timed else 0)
                try:
                    if kind:
                        tr.set_projection_params(PO.scene_projection(sc, kind, False, lon_range=np.radians(120.0), lat_range=np.radians(60.0)).params())
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
            lines.append(f"{name}, {sc.num_triangles} triangles, {W}x{H} @ {spp} spp, {label:15s}: frame median {med(walls):.3f} ms "
                         f"(min {min(walls):.3f}, n {a.reps}); {timers}")
            print(lines[-1], flush=True)
    lines.append(KERNELS)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
