"""The quality table of DESIGN.md section 10k: temporal reuse across mesh deformation on the CPU restatements
(polaris_host_reproject_deform, _reproject_motion, _temporal_combine) over oracle traces of the two-instance Cornell box of
tests/vertex_motion_oracle.py at 128^2.

    python scripts/vertex_motion_quality.py > profiles/vertex_motion_quality.txt

A history of 64 spp at step 0, then 1 spp at each of eight steps; at every step the tall block is deformed anew by
tests/vertex_update_cases.deformed (0.04 of its extent, another seed per step), the room and the camera stand still; RMSE of the
unfiltered TEMPORAL plane against 1024 spp at the same step.  Settings: (a) the history reprojected with vertex motion; (b) the
update without the option -- the history dropped, the plain 1 spp mean; (c) the history kept but reprojected with object motion's
rigid arithmetic only (the block's pixels take the history of the same pixel, whatever the surface there was).  Pixel sets: all
filtered pixels, and those of the deformed block (instance 1).  The room's pixels next to the block carry section 10d's
stale-lighting limitation: they keep the history's shading of a block that has changed its shape."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from polaris_amd.hostinfo import size_openmp  # noqa: E402

size_openmp()

import vertex_motion_oracle as VO  # noqa: E402
from oracle import pybind as ob  # noqa: E402
from polaris_amd import host_api  # noqa: E402

STEPS = 8


def main():
    res = VO.quality_run(host_api, ob.Oracle("oracle"), STEPS, report=tuple(range(1, STEPS + 1)))
    print(f"{'step':>4s} {'set':8s} {'pixels':>6s} {'(a) deform':>10s} {'(b) 1 spp':>10s} {'(c) rigid':>10s} {'a/b':>6s} {'a/c':>6s} {'reused':>6s}")
    for k in range(1, STEPS + 1):
        r = res[k]
        for name in ("all", "block"):
            a, b, c = r["a"][name], r["b"][name], r["c"][name]
            print(f"{k:4d} {name:8s} {r['pixels'][name]:6d} {a:10.4f} {b:10.4f} {c:10.4f} {a / b:6.3f} {a / c:6.3f} "
                  f"{r['reused'] if name == 'block' else float('nan'):6.3f}", flush=True)


if __name__ == "__main__":
    main()
