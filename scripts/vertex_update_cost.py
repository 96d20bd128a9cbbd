"""Wall time of polaris_hip_update_vertices against a full upload_scene of the same refit arrays (profiles/vertex_update_cost.txt),
on the 1 M-triangle terrain (scenes.unique_stress(708)), the 58 K-triangle material ball and the Cornell box.

    python scripts/vertex_update_cost.py --reps 20 [--upload-reps 6] [--resource-report build.log]

Per scene: the median wall time of polaris_hip_update_vertices (synchronous: the device is drained when it returns) over --reps calls
that alternate between two deformations, the median wall time of polaris_hip_upload_scene of the same two refit scenes on a SECOND
tracer that has the option "vertex_update" off (so the upload pays for no plan) over --upload-reps calls, their ratio, and the
time_kernels medians of the timers "tri_records", "refit_mesh", "instance_extent", "repad" and "refit_top" per call.  Both legs time the
C entry alone: the ctypes structs are made before the clock starts.  The only condition is that the update is the faster one on every
scene; the script exits with status 1 otherwise.

--resource-report: a build log made with EXTRA=-Rpass-analysis=kernel-resource-usage (make -C polaris_amd/csrc); the VGPRs, scratch
bytes (which must be 0) and waves per SIMD of the two new kernels are copied from it.
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TIMERS = ("tri_records", "refit_mesh", "instance_extent", "repad", "refit_top")


def deformed(sc, seed):
    """`sc` with every vertex displaced by a smooth seeded field of 0.5 % of the scene's extent (welded vertices stay welded)."""
    from polaris_amd import scenes

    rng = np.random.default_rng(seed)
    p = sc.vertices[:, :3].astype(np.float64)
    ext = float(np.ptp(p, axis=0).max())
    v = sc.vertices.copy()
    for k in range(3):
        f, ph = rng.uniform(2.0, 7.0, size=3) / ext, rng.uniform(0, 6.28)
        v[:, k] = (p[:, k] + 0.005 * ext * np.sin(p @ f + ph)).astype(np.float32)
    return scenes.refit_vertices(sc, v)


def resource_lines(path):
    text = open(path).read()
    out = []
    for kernel in ("k_tri_records", "k_refit_mesh"):
        m = re.search(r"Function Name: \S*" + kernel + r"\S*.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", text, re.S)
        if not m:
            out.append(f"{kernel}: not in {os.path.basename(path)}")
            continue
        out.append(f"{kernel}: {m.group(1)} VGPRs, {m.group(2)} bytes of scratch, {m.group(3)} waves per SIMD")
        if int(m.group(2)) != 0:
            raise SystemExit(f"{kernel} uses scratch memory")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upload-reps", type=int, default=6)
    ap.add_argument("--terrain", type=int, default=708, help="grid size n of the terrain: 2 n^2 triangles")
    ap.add_argument("--resource-report", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_update_cost.txt"))
    a = ap.parse_args()
    import ctypes as C

    from conftest import make_hip_tracer
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines, ok = [], True
    for name, make in (("terrain", lambda: scenes.unique_stress(a.terrain)), ("material_ball", scenes.material_ball), ("cornell_box", scenes.cornell_box)):
        base = make()
        steps = [deformed(base, 1), deformed(base, 2)]
        structs = [T.vertex_update(*scenes.vertex_update_args(s)) for s in steps]          # (u, arrays it borrows)
        views = [T.scene_view(x) for x in steps]
        tr = make_hip_tracer(base, 64, 64, time_kernels=1, vertex_update=1)
        plain = make_hip_tracer(base, 64, 64)                     # the upload leg: a tracer with the option off
        try:
            lib, clock = tr._lib, time.perf_counter
            for s in range(2):                      # warm-up: first launches, first upload of each array
                assert lib.polaris_hip_update_vertices(tr._h, C.byref(structs[s][0])) == 0
                assert lib.polaris_hip_upload_scene(plain._h, C.byref(views[s])) == 0
            for k in TIMERS:
                tr.kernel_ms(k)
            upd, up, kern = [], [], {k: [] for k in TIMERS}
            for r in range(a.reps):
                t0 = clock()
                rc = lib.polaris_hip_update_vertices(tr._h, C.byref(structs[r % 2][0]))
                upd.append((clock() - t0) * 1e3)
                assert rc == 0
                for k in kern:                  # (reading a timer resets it)
                    kern[k].append(tr.kernel_ms(k)[0])
            for r in range(a.upload_reps):
                t0 = clock()
                rc = lib.polaris_hip_upload_scene(plain._h, C.byref(views[r % 2]))
                up.append((clock() - t0) * 1e3)
                assert rc == 0
        finally:
            tr.Close()
            plain.Close()
        ratio = med(up) / med(upd)
        ok = ok and med(upd) < med(up)
        lines.append(f"{name}: {len(base.mesh_instances)} instances, {base.num_triangles} triangles: update_vertices median {med(upd):.3f} ms "
                     f"(min {min(upd):.3f}, n {a.reps}), upload_scene of the refit arrays median {med(up):.3f} ms (min {min(up):.3f}, n {a.upload_reps}), "
                     f"upload / update = {ratio:.1f}; " + ", ".join(f"{k} {med(v):.4f} ms" for k, v in kern.items()) + " per call")
        print(lines[-1], flush=True)
    if a.resource_report:
        lines += resource_lines(a.resource_report)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("update_vertices is not faster than upload_scene")


if __name__ == "__main__":
    main()
