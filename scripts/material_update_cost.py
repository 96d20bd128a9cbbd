"""Wall time of polaris_hip_update_materials against a full upload_scene of the same substituted arrays
(profiles/material_update_cost.txt), on the 1 M-triangle terrain (scenes.unique_stress(708)), the 58 K-triangle material ball and the
Cornell box.

    python scripts/material_update_cost.py --reps 20 [--upload-reps 6] [--resource-report build.log]

Per scene and per edit -- `nodes`: only the node table changes (a leaf alternates between a recoloured diffuse and a rough conductor,
so the classes change and every record is rewritten); `nodes+index`: the call also passes material_index (alternating between the
scene's and a rotated copy) -- the median wall time of polaris_hip_update_materials (synchronous: the device is drained when it
returns) over --reps calls that alternate between the two edits, the median wall time of polaris_hip_upload_scene of the same two
substituted scenes on a SECOND tracer over --upload-reps calls, their ratio, and the time_kernels median of the timer "retag" per
call.  Both legs time the C entry alone: the ctypes structs are made before the clock starts.  The only condition is that the update is
the faster one on every scene and edit; the script exits with status 1 otherwise.

--resource-report: a build log made with EXTRA=-Rpass-analysis=kernel-resource-usage (make -C polaris_amd/csrc); the VGPRs, scratch
bytes (which must be 0) and waves per SIMD of k_retag are copied from it.
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


def edits(base):
    """Two node tables and two material_index arrays to alternate between."""
    from polaris_amd import ctypes_api as T

    roots = np.unique(base.material_index)
    leaf = int(next(i for i in roots if base.material_nodes["type"][i] == T.BXDF_DIFFUSE))
    a, b = base.material_nodes.copy(), base.material_nodes.copy()
    a["k"][leaf][:3] = (0.3, 0.5, 0.7)
    b["type"][leaf], b["scale"][leaf], b["int_ior"][leaf] = T.BXDF_ROUGH_CONDUCTOR, 0.3, 0.0
    return (a, b), (base.material_index.copy(), np.roll(base.material_index, 7))


def resource_lines(path):
    text = open(path).read()
    m = re.search(r"Function Name: \S*k_retag\S*.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", text, re.S)
    if not m:
        return [f"k_retag: not in {os.path.basename(path)}"]
    if int(m.group(2)) != 0:
        raise SystemExit("k_retag uses scratch memory")
    return [f"k_retag: {m.group(1)} VGPRs, {m.group(2)} bytes of scratch, {m.group(3)} waves per SIMD"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upload-reps", type=int, default=6)
    ap.add_argument("--terrain", type=int, default=708, help="grid size n of the terrain: 2 n^2 triangles")
    ap.add_argument("--resource-report", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material_update_cost.txt"))
    a = ap.parse_args()
    import ctypes as C

    from conftest import make_hip_tracer
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines, ok = [], True
    for name, make in (("terrain", lambda: scenes.unique_stress(a.terrain)), ("material_ball", scenes.material_ball), ("cornell_box", scenes.cornell_box)):
        base = make()
        tables, indices = edits(base)
        for edit in ("nodes", "nodes+index"):
            steps = [scenes.with_materials(base, nodes=tables[s], material_index=indices[s] if edit == "nodes+index" else None) for s in range(2)]
            structs = [T.material_update(tables[s], indices[s] if edit == "nodes+index" else None, base.scene_diffuse_mat_index) for s in range(2)]
            views = [T.scene_view(x) for x in steps]
            tr = make_hip_tracer(base, 64, 64, time_kernels=1)
            plain = make_hip_tracer(base, 64, 64)                     # the upload leg
            try:
                lib, clock = tr._lib, time.perf_counter
                for s in range(2):                      # warm-up: first launches, first upload of each array
                    assert lib.polaris_hip_update_materials(tr._h, C.byref(structs[s][0])) == 0
                    assert lib.polaris_hip_upload_scene(plain._h, C.byref(views[s])) == 0
                tr.kernel_ms("retag")
                upd, up, kern = [], [], []
                for r in range(a.reps):
                    t0 = clock()
                    rc = lib.polaris_hip_update_materials(tr._h, C.byref(structs[r % 2][0]))
                    upd.append((clock() - t0) * 1e3)
                    assert rc == 0
                    kern.append(tr.kernel_ms("retag")[0])        # (reading a timer resets it)
                for r in range(a.upload_reps):
                    t0 = clock()
                    rc = lib.polaris_hip_upload_scene(plain._h, C.byref(views[r % 2]))
                    up.append((clock() - t0) * 1e3)
                    assert rc == 0
                same = tr.read_triangle_records().tobytes() == plain.read_triangle_records().tobytes() and tr.read_shading_record() == plain.read_shading_record()
            finally:
                tr.Close()
                plain.Close()
            if not same:
                raise SystemExit(f"{name}, {edit}: the updated records differ from the uploaded ones")
            ok = ok and med(upd) < med(up)
            lines.append(f"{name}, {edit}: {base.num_triangles} triangles, {len(base.material_nodes)} material nodes: update_materials median {med(upd):.3f} ms "
                         f"(min {min(upd):.3f}, n {a.reps}), upload_scene of the substituted arrays median {med(up):.3f} ms (min {min(up):.3f}, n {a.upload_reps}), "
                         f"upload / update = {med(up) / med(upd):.1f}; retag {med(kern):.4f} ms per call")
            print(lines[-1], flush=True)
    if a.resource_report:
        lines += resource_lines(a.resource_report)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("update_materials is not faster than upload_scene")


if __name__ == "__main__":
    main()
