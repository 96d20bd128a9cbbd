"""The quality table of DESIGN.md section 10d: temporal reuse across moving mesh instances on the CPU restatements
(polaris_host_reproject_motion, _reproject, _temporal_combine) over oracle traces of scenes.moving_instances at 128^2.

    python scripts/motion_quality.py > profiles/motion_quality.txt

A history of 64 spp at step 0, then 1 spp at each of eight steps (the tall block turns by 0.05 rad, the short one shifts by 0.03 per
step, the camera stands still); RMSE of the unfiltered TEMPORAL plane against 1024 spp at the same step.  Settings: (a) the history
reprojected with object motion; (b) today's upload -- the history dropped, the plain 1 spp mean; (c) the history kept but reprojected
with the camera-only arithmetic (it ghosts: the blocks' old pixels are blended into their new ones).  Pixel sets: all filtered pixels,
those of the two blocks (instances 1 and 2), and those that showed a block at an earlier step and show the room now.  The vacated
pixels carry the stale-lighting limitation: the room keeps the history's shading of a floor the block has left."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from polaris_amd.hostinfo import size_openmp  # noqa: E402

size_openmp()

import motion_oracle as MO  # noqa: E402
from oracle import pybind as ob  # noqa: E402
from polaris_amd import host_api  # noqa: E402

STEPS = 8


def main():
    res = MO.quality_run(host_api, ob.Oracle("oracle"), STEPS, report=tuple(range(1, STEPS + 1)))
    print(f"{'step':>4s} {'set':8s} {'pixels':>6s} {'(a) motion':>10s} {'(b) 1 spp':>10s} {'(c) camera':>10s} {'a/b':>6s} {'a/c':>6s} {'reused':>6s}")
    for k in range(1, STEPS + 1):
        r = res[k]
        for name in ("all", "moved", "vacated"):
            a, b, c = r["a"][name], r["b"][name], r["c"][name]
            print(f"{k:4d} {name:8s} {r['pixels'][name]:6d} {a:10.4f} {b:10.4f} {c:10.4f} {a / b:6.3f} {a / c:6.3f} "
                  f"{r['reused'] if name == 'moved' else float('nan'):6.3f}", flush=True)


if __name__ == "__main__":
    main()
