"""Wall time of polaris_hip_update_instances against a full upload_scene of the same refit arrays
(profiles/instance_update_cost.txt), on scenes.moving_instances and scenes.instanced_stress (1 024 instances).

    python scripts/instance_update_cost.py --reps 20 [--resource-report build.log]

Per scene: the median wall time of polaris_hip_update_instances (synchronous: the device is drained when it returns) over --reps
calls that alternate between two sets of matrices, the median wall time of polaris_hip_upload_scene of the same two refit scenes on
a SECOND tracer that has the option "instance_update" off (so the upload pays for no plan), their ratio, and the time_kernels medians
of the timers "instance_extent", "repad" and "refit_top" per call.  Both legs time the C entry alone: the ctypes structs are made
before the clock starts.  The condition is that the update is the faster one on both scenes; the script exits with status 1
otherwise.

--resource-report: a build log made with EXTRA=-Rpass-analysis=kernel-resource-usage (make -C polaris_amd/csrc); the VGPRs, scratch
bytes (which must be 0) and waves per SIMD of the three kernels are copied from it.
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


def nudged(sc, step):
    """`sc` with every instance but the first translated by a small seeded offset (matrices and leaf boxes follow): a moved step."""
    from polaris_amd import scenes

    rng = np.random.default_rng(step)
    out = scenes.refit_instances(sc, sc)
    boxes = scenes.instance_boxes(sc)
    inv = out.mesh_instances["inv_transform"].reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)   # row major
    off = rng.uniform(-0.05, 0.05, size=(len(inv), 3)) * step
    off[0] = 0.0
    fwd = np.linalg.inv(inv)
    fwd[:, :3, 3] += off
    out.mesh_instances["inv_transform"] = np.linalg.inv(fwd).transpose(0, 2, 1).reshape(-1, 16).astype(np.float32)
    boxes[:, :3] += off.astype(np.float32)
    boxes[:, 3:] += off.astype(np.float32)
    idx, _ = scenes._top_level_nodes(out)
    leaf = idx[out.bvh_nodes["ldata"][idx] <= 0]
    inst = -out.bvh_nodes["ldata"][leaf].astype(np.int64)
    out.bvh_nodes["min"][leaf], out.bvh_nodes["max"][leaf] = boxes[inst, :3], boxes[inst, 3:]
    return scenes.refit_instances(out, out)


def resource_lines(path):
    text = open(path).read()
    out = []
    for kernel in ("k_instance_extent", "k_repad", "k_refit_top"):
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
    ap.add_argument("--resource-report", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_update_cost.txt"))
    a = ap.parse_args()
    import ctypes as C

    from conftest import make_hip_tracer
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines, ok = [], True
    for name, base in (("moving_instances", scenes.moving_instances(0)), ("instanced_stress", scenes.instanced_stress())):
        steps = [nudged(base, 1), nudged(base, 2)]
        args = [scenes.instance_update_args(s) for s in steps]
        structs = [T.instance_update(*x) for x in args]          # (u, arrays it borrows)
        views = [T.scene_view(x) for x in steps]
        tr = make_hip_tracer(base, 64, 64, time_kernels=1, instance_update=1)
        plain = make_hip_tracer(base, 64, 64)                     # the upload leg: a tracer with the option off
        try:
            lib, clock = tr._lib, time.perf_counter
            for s in range(2):                      # warm-up: first launches, first upload of each array
                assert lib.polaris_hip_update_instances(tr._h, C.byref(structs[s][0])) == 0
                assert lib.polaris_hip_upload_scene(plain._h, C.byref(views[s])) == 0
            for k in ("instance_extent", "repad", "refit_top"):
                tr.kernel_ms(k)
            upd, up, kern = [], [], {"instance_extent": [], "repad": [], "refit_top": []}
            for r in range(a.reps):
                t0 = clock()
                rc = lib.polaris_hip_update_instances(tr._h, C.byref(structs[r % 2][0]))
                upd.append((clock() - t0) * 1e3)
                assert rc == 0
                for k in kern:
                    kern[k].append(tr.kernel_ms(k)[0])
            for r in range(a.reps):
                t0 = clock()
                rc = lib.polaris_hip_upload_scene(plain._h, C.byref(views[r % 2]))
                up.append((clock() - t0) * 1e3)
                assert rc == 0
        finally:
            tr.Close()
            plain.Close()
        ratio = med(up) / med(upd)
        ok = ok and med(upd) < med(up)
        lines.append(f"{name}: {len(base.mesh_instances)} instances, {base.num_triangles} triangles: update_instances median {med(upd):.3f} ms "
                     f"(min {min(upd):.3f}), upload_scene of the refit arrays median {med(up):.3f} ms (min {min(up):.3f}), upload / update = {ratio:.1f}; "
                     + ", ".join(f"{k} {med(v):.4f} ms" for k, v in kern.items()) + f" per call; n {a.reps}")
        print(lines[-1], flush=True)
    if a.resource_report:
        lines += resource_lines(a.resource_report)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("update_instances is not faster than upload_scene")


if __name__ == "__main__":
    main()
