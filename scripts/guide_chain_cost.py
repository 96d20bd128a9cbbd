"""Device time of the G-buffer pass with the option "guide_specular" = N (profiles/guide_chain_cost.txt): the
"gbuffer" timer with time_kernels = 1, medians of --reps recomputations (each after a set_camera), per scene, size and N, next to
the share of pixels whose guide ray follows at least one link -- the pixels whose first-hit leaf is a CONDUCTOR or a DIELECTRIC.

    python scripts/guide_chain_cost.py --sizes 512 1024 --links 0 1 4 8 --reps 9 --out profiles/guide_chain_cost.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--links", type=int, nargs="+", default=[0, 1, 4, 8])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scenes", nargs="+", default=["mirror-room", "cornell", "material-ball"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_chain_cost.txt"))
    a = ap.parse_args()
    from conftest import make_hip_tracer
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes

    lines = []
    for name in a.scenes:
        sc = scenes.mirror_room() if name == "mirror-room" else scenes.SCENES[name]()
        for n in a.sizes:
            tr = make_hip_tracer(sc, n, n, time_kernels=1)
            try:
                leaf = np.ascontiguousarray(tr.read_aov(T.AOV_ALBEDO)[..., 3]).view(np.int32)
                share = float(np.isin(leaf, (T.BXDF_CONDUCTOR, T.BXDF_DIELECTRIC)).mean())
                cells = []
                for links in a.links:
                    tr.set_option("guide_specular", links)
                    tr.read_aov(T.AOV_GUIDE)                      # (the first launch of a kernel loads its code)
                    tr.kernel_ms("gbuffer")
                    ms = []
                    for _ in range(a.reps):
                        tr.UpdateState(0, 2, sc)                  # set_camera: the next read recomputes the G-buffer
                        tr.read_aov(T.AOV_GUIDE)
                        ms.append(tr.kernel_ms("gbuffer")[0])
                    cells.append(f"N={links} {sorted(ms)[len(ms) // 2]:.4f} ms (min {min(ms):.4f}) {tr.kernel_symbol('gbuffer')}")
            finally:
                tr.Close()
            lines.append(f"{sc.name} {n}x{n}, {sc.num_triangles} triangles, {100 * share:.2f} % of the pixels follow a link: " + "; ".join(cells)
                         + f"; medians of {a.reps}")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
