"""Scenes whose layout needs an EXACT number of traversal-stack entries, and rays that hold them all (TEST INFRASTRUCTURE).

The host promises every traversal kernel that no ray needs more stack than the upload planned ("The stack
contract"): scene_layout.h reports max_stack = need + 1 and refuses a scene above 32, select_trace picks k_trace<*, 16 | 24 | 32, *>
from it, plan_tiny_lds gives the tiny-scene mode exactly that many 16-bit rows, traverse<> and the packet kernel keep 32.  A
miscount by one row faults nowhere -- it overwrites LDS that belongs to somebody else, and only the rays at the deep end get a wrong
hit.  These scenes sit on every boundary (S = 15, 16 | 17, 24 | 25, 31, 32, and 33 which must be refused) and their rays reach the
deep end (counted on the CPU in tests/test_stack_scenes_cpu.py).

All of them are HAND-MADE BVH chains in the reference's node encoding (optimized_scene.go:14-64; any tree whose boxes bound their
contents is a valid input): camera-facing triangles ("shells") at z = -0.05 x 1.6^k, each 1.6^k big, seen from (0, 0, 1) -- the
angular size grows with k, so a line from the eye through the innermost shell's bounding rectangle crosses every box of the chain.
Inner node j = { leaf of the outermost remaining shell, node j + 1 }: both children lie on such a ray, the nearer one (the rest
of the chain) is taken first and the far leaf is pushed -- one entry per level.

* `single(S)`: ONE identity instance of a chain of S - 1 leaves -> max_stack = S; a ray holds up to S - 2 entries (the scene's one
  instance is entered without an exit marker).  The innermost shell is the light and faces the others.
* `instanced(S)`: a top-level chain of four instances -- three one-triangle decoys behind the outermost shell (apex down, twice as wide), whose
  leaves stay pending, and, as the last and deepest top-level leaf, the chain mesh of S - 4 leaves under a rotation about z plus a translation
  (the world-space ray restored at the exit marker shows in the result) -> max_stack = S; a ray holds up to S - 1 entries
  (3 pending decoys + the exit marker + S - 5 pending shells).
* `mirror`: the rest of the chain hangs in ldata and the split-off leaf in rdata (the plain scenes: the other way round), in the
  top-level chain too.  Any-hit traversal in stored order (k_trace<true, ...>) then descends the chain first and holds the whole
  depth; in a plain scene it takes the leaf first and holds one entry.
* `retry`: single(32) whose deepest leaf holds twelve small triangles.  max_leaf_tris = 1 would subdivide that leaf four levels
  further, past 32 entries: the upload must fall back to the unsplit tree (scene_layout.h "@retry-without-subdivision").

Only polaris_amd.scenes, tie_scenes and seeded numpy.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import tie_scenes as TS  # noqa: E402

F32 = np.float32
FLT_MAX = TS.FLT_MAX
GROWTH = 1.6
EYE = (0.0, 0.0, 1.0)
DECOYS = 3          # instanced: pending top-level siblings of the chain instance
N_LINES = 80


def _nested_shells_scene(n=22):
    """A tree whose rays NEED a deep stack: n camera-facing triangles at z = -0.05 x 1.6^k, each 1.6^k big (every camera ray's line
    crosses every one of their boxes), under a HAND-MADE BVH in the reference's encoding (optimized_scene.go:14-64): a chain that splits
    the outermost triangle off per level -- node j = { leaf of triangle n-1-j, node j+1 }.  Both children of every node lie on a camera
    ray; the traversal takes the nearer one (the rest of the chain) first and pushes the far leaf: one stack entry per level, n - 1 = 21
    of them, well beyond the 16 the spill variant keeps in LDS.  (Any tree whose boxes bound their contents is a valid input.)  A light
    behind the camera faces the shells: the innermost one is lit, its shadow rays walk the same chain."""
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes

    tris = []
    for k in range(n):
        sz, z = 0.15 * 1.6 ** k, -0.05 * 1.6 ** k
        tris.append([[-sz, -sz, z], [sz, -sz, z], [0.0, 1.5 * sz, z]])
    tris.append([[-2.0, -2.0, 3.0], [0.0, 3.0, 3.0], [2.0, -2.0, 3.0]])      # the light: behind the camera, facing the shells (-z)
    n += 1
    verts = np.asarray(tris, np.float32)
    mt = scenes.MaterialTable()
    d, e = mt.diffuse((0.6, 0.7, 0.8)), mt.emissive((3, 3, 3))
    mat = np.full(n, d, np.uint32)
    mat[-1] = e
    mesh = scenes.Mesh(verts, scenes._flat_normals(verts), np.zeros((n, 3, 2), np.float32), mat)
    sc = scenes.compile_scene([mesh], [(0, np.eye(4))], mt, max_leaf=1, name="nested-shells")
    sc.set_camera(eye=(0.0, 0.0, 1.0), look=(0.0, 0.0, -1.0), fov=0.4, aspect=4 / 3)
    v = sc.vertices[:, :3].reshape(n, 3, 3)
    order = np.argsort(-v[:, 0, 2], kind="stable")   # compiled triangle indices, nearest (largest z) first
    nodes = np.zeros(2 * n, T.BVH_NODE)
    lo, hi = v.min(axis=1), v.max(axis=1)
    nodes[0] = (lo.min(axis=0), 0, hi.max(axis=0), 0)                         # the top-level tree: one leaf = instance 0
    for k in range(n):                                                        # leaf of the k-th nearest triangle: node n + k
        t = int(order[k])
        nodes[n + k] = (lo[t], -t, hi[t], 1)
    for j in range(n - 1):                                                    # inner node j: node 1 + j over the j-th .. nearest triangles
        members = order[: n - j]
        far_leaf = n + (n - 1 - j)
        rest = 1 + j + 1 if j + 1 < n - 1 else n + 0                          # the last inner node holds the two nearest leaves
        nodes[1 + j] = (lo[members].min(axis=0), far_leaf, hi[members].max(axis=0), rest)
    sc.bvh_nodes = nodes
    sc.mesh_instances["bvh_root"] = 1
    return sc


# ---- chains of an exact stack need -------------------------------------------------------------------------------------------
def shell_z(k):
    return -0.05 * GROWTH ** k


def shell_rect(k):
    """(x0, x1, y0, y1) of shell k's bounding rectangle in its plane z = shell_z(k)."""
    sz = 0.15 * GROWTH ** k
    return -sz, sz, -sz, 1.5 * sz


def _shell(k, away=False, apex_down=False, wide=1.0):
    """Shell k: one triangle facing the eye (+z), its apex up; away: facing the other shells (-z); apex_down: the same rectangle's
    other triangle, which covers the two upper corners; wide: the rectangle scaled in its plane."""
    x0, x1, y0, y1 = (wide * c for c in shell_rect(k))
    z = shell_z(k)
    t = [[x0, y1, z], [0.0, y0, z], [x1, y1, z]] if apex_down else [[x0, y0, z], [x1, y0, z], [0.0, y1, z]]
    return [t[0], t[2], t[1]] if away else t


def _patches():
    """Twelve small triangles on shell 0's plane, one per cell of a 4 x 3 grid over its rectangle (the deepest leaf of `retry`)."""
    x0, x1, y0, y1 = shell_rect(0)
    z, dx, dy = shell_z(0), (x1 - x0) / 4, (y1 - y0) / 3
    out = []
    for j in range(3):
        for i in range(4):
            cx, cy = x0 + (i + 0.5) * dx, y0 + (j + 0.5) * dy
            out.append([[cx - 0.4 * dx, cy - 0.4 * dy, z], [cx, cy + 0.4 * dy, z], [cx + 0.4 * dx, cy - 0.4 * dy, z]])   # (facing -z, as the light does)
    return out


def chain_transform():
    """The chain instance's world matrix in `instanced`: a rotation about z (the shells turn in their planes) plus a translation."""
    c, s = math.cos(0.3), math.sin(0.3)
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    m[:3, 3] = (0.01, -0.015, 0.005)
    return m


def _chain_nodes(items, base, mirror):
    """A chain over `items` = [(lo, hi, ldata, rdata) of a leaf], nearest first, as node records from index `base` on: inner node j
    (index base + j) = { leaf of the farthest remaining item, inner node j + 1 }, the last one holds the two nearest leaves; the
    leaves follow the inner nodes.  mirror: the rest of the chain in ldata, the leaf in rdata.  One item: just its leaf."""
    n = len(items)
    leaf_at = lambda i: base + (n - 1) + i  # noqa: E731
    out = []
    for j in range(n - 1):
        lo = np.min([it[0] for it in items[: n - j]], axis=0)
        hi = np.max([it[1] for it in items[: n - j]], axis=0)
        far, rest = leaf_at(n - 1 - j), (base + j + 1 if j + 1 < n - 1 else leaf_at(0))
        out.append((lo, rest, hi, far) if mirror else (lo, far, hi, rest))
    out.extend((lo, ldata, hi, rdata) for lo, hi, ldata, rdata in items)
    return out


def chain_scene(leaves, *, instanced=False, mirror=False, bottom=1, name="chain"):
    """A chain mesh of `leaves` leaves -- the deepest one holds `bottom` triangles on shell 0's plane (one: the light, which IS shell
    0), the others shells 1 .. leaves - 1 -- as the scene's one identity instance, or (instanced) under chain_transform() as the
    deepest leaf of a top-level chain whose other DECOYS leaves are one-triangle meshes behind the outermost shell."""
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes as S

    mt = S.MaterialTable()
    tints = [mt.diffuse((0.8, 0.3, 0.2)), mt.diffuse((0.2, 0.7, 0.3)), mt.diffuse((0.3, 0.4, 0.8))]
    light, back = mt.emissive((4.0, 3.5, 3.0), 2.0), mt.diffuse((0.6, 0.6, 0.6))

    def mesh(tris, mats):
        v = np.asarray(tris, np.float64)
        return S.Mesh(v, S._flat_normals(v), np.zeros((len(v), 3, 2)), np.asarray(mats, np.uint32))

    first = [_shell(0, away=True)] if bottom == 1 else _patches()
    chain = mesh(first + [_shell(k) for k in range(1, leaves)], [light] + [tints[i % 3] for i in range(1, bottom)] + [tints[k % 3] for k in range(1, leaves)])
    meshes, insts = [chain], [(0, chain_transform() if instanced else np.eye(4))]
    if instanced:
        meshes += [mesh([_shell(leaves + 1 + i, apex_down=True, wide=2.0)], [back]) for i in range(DECOYS)]   # (apex down and twice as wide: a ray through an upper corner of the shells' rectangles misses them all and hits a decoy)
        insts = [(1 + i, np.eye(4)) for i in range(DECOYS)] + insts          # instances 0 .. 2: the decoys; the chain is the last
    # (leaves of 64: compile_scene keeps every mesh's triangles in the order given; the trees are replaced below)
    sc = S.compile_scene(meshes, insts, mt, max_leaf=64, scene_diffuse=mt.diffuse((0.05, 0.06, 0.1)), name=name)
    sc.set_camera(eye=EYE, look=(0.0, 0.0, -1.0), fov=0.4, aspect=4 / 3)

    v = sc.vertices[:, :3].reshape(-1, 3, 3)
    lo, hi = v.min(axis=1), v.max(axis=1)
    # the chain mesh's leaves, nearest first (its triangles come first in the scene's arrays)
    items = [(lo[:bottom].min(axis=0), hi[:bottom].max(axis=0), 0, bottom)]
    items += [(lo[t], hi[t], -t, 1) for t in range(bottom, bottom + leaves - 1)]
    n_top = 2 * len(insts) - 1
    mesh_nodes = _chain_nodes(items, n_top, mirror)
    roots = {0: n_top}
    for i in range(1, len(meshes)):                                            # a decoy's tree is one leaf
        t = len(chain.mat) + i - 1
        roots[i] = n_top + len(mesh_nodes)
        mesh_nodes.append((lo[t], -t, hi[t], 1))
    # the top-level chain, nearest first: the chain instance, then the decoys from the nearest to the farthest; world-space boxes
    # (padded by 2^-10 of their size: the instance's vertices go through a float32 matrix)
    top = []
    for k in [len(insts) - 1] + list(range(len(insts) - 1)):
        m, xf = insts[k]
        w = meshes[m].verts.reshape(-1, 3) @ np.asarray(xf)[:3, :3].T + np.asarray(xf)[:3, 3]
        pad = (w.max(axis=0) - w.min(axis=0)).max() * 2.0 ** -10
        top.append(((w.min(axis=0) - pad).astype(F32), (w.max(axis=0) + pad).astype(F32), -k, 0))
    nodes = _chain_nodes(top, 0, mirror) + mesh_nodes
    sc.bvh_nodes = np.array([(np.asarray(a, F32), int(l), np.asarray(b, F32), int(r)) for a, l, b, r in nodes], T.BVH_NODE)
    for k, (m, _) in enumerate(insts):
        sc.mesh_instances[k]["bvh_root"] = roots[m]
    sc.bvh_max_depth = len(insts) - 1 + 1 + leaves - 1
    return sc


def single(S, mirror=False):
    return chain_scene(S - 1, mirror=mirror, name=f"single-{S}" + ("-mirror" if mirror else ""))


def instanced(S, mirror=False):
    return chain_scene(S - 1 - DECOYS, instanced=True, mirror=mirror, name=f"instanced-{S}" + ("-mirror" if mirror else ""))


def retry():
    return chain_scene(31, bottom=12, name="retry")


# ---- rays --------------------------------------------------------------------------------------------------------------------
def stack_rays(leaves, instanced=False, seed=0):
    """512 rays of a chain scene: N_LINES lines from the eye -- through random points of shell 0's rectangle, through its corners
    (exactly and just inside: they miss every triangle of the first shells and cross every box), through corners of the next two
    rectangles, and through the upper corners of the two outermost ones (they cross the outer boxes, miss every shell and hit
    nothing -- or, instanced, a decoy after the chain instance has been left) -- as rays from the eye, reversed from
    beyond the outermost shell, and starting between two shells in either direction; every ray with maxDist = FLT_MAX and with a
    finite one."""
    rng = np.random.default_rng(0x57AC + 97 * leaves + seed)
    x0, x1, y0, y1 = shell_rect(0)
    pts = [(rng.uniform(x0, x1), rng.uniform(y0, y1), shell_z(0)) for _ in range(56)]
    for f in (1.0, 0.999):
        pts += [(f * x, f * y, shell_z(0)) for x in (x0, x1) for y in (y0, y1)]
    for k in (1, 2):
        a0, a1, b0, b1 = shell_rect(k)
        pts += [(0.999 * x, 0.999 * y, shell_z(k)) for x in (a0, a1) for y in (b0, b1)]
    for k in (leaves - 1, leaves - 2):                         # upper corners of the two outermost rectangles: they miss every shell
        a0, a1, b0, b1 = shell_rect(k)
        pts += [(f * x, f * b1, shell_z(k)) for x in (a0, a1) for f in (0.999, 0.99)]
    assert len(pts) == N_LINES
    p = np.asarray(pts, np.float64)
    if instanced:
        xf = chain_transform()
        p = p @ xf[:3, :3].T + xf[:3, 3]
    e = np.asarray(EYE, np.float64)
    d = p - e
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    at_z = lambda z: e + d * ((z - e[2]) / d[:, 2])[:, None]  # noqa: E731  (the lines' points in the plane z)
    far = 1.25 * shell_z(leaves - 1)                          # beyond the outermost shell (and, instanced, in front of the decoys)
    pick = rng.integers(0, N_LINES, 96)
    gap = rng.integers(0, leaves - 1, 96)
    between = 0.5 * (np.array([shell_z(k) for k in gap]) + np.array([shell_z(k + 1) for k in gap]))
    sign = np.where(np.arange(96) % 2 == 0, 1.0, -1.0)[:, None]
    o = np.concatenate([np.broadcast_to(e, d.shape), at_z(far), (e + d[pick] * ((between - e[2]) / d[pick, 2])[:, None])])
    dirs = np.concatenate([d, -d, sign * d[pick]])
    rays = TS._rays(o, dirs)
    short = rays.copy()
    short[:, 3] = (abs(far) * 10.0 ** rng.uniform(-2.0, 0.5, len(rays))).astype(F32)
    return np.concatenate([rays, short])


# ---- the cases the CPU and GPU tests share -----------------------------------------------------------------------------------
TARGETS = (15, 16, 17, 24, 25, 31, 32)
CASES = {}
for _family in ("single", "instanced"):
    for _S in TARGETS + (33,):
        for _mirror in ((False, True) if _S <= 32 else (False,)):
            CASES[f"{_family}-{_S}" + ("-mirror" if _mirror else "")] = dict(family=_family, S=_S, mirror=_mirror, leaves=_S - 1 - (DECOYS if _family == "instanced" else 0))
CASES["retry"] = dict(family="single", S=32, mirror=False, leaves=31)
REFUSED = [t for t, c in CASES.items() if c["S"] > 32]            # the layout needs 33 entries: the upload refuses them
TRACED = [t for t in CASES if t not in REFUSED]


def held(tag):
    """The entries a ray of the case can hold at most: S - 1 with several instances, S - 2 where the scene is one instance (entered
    without an exit marker)."""
    c = CASES[tag]
    return c["S"] - (1 if c["family"] == "instanced" else 2)


def orders(tag):
    """The walks (layout_check_high_water's `order`) in which the case's rays must reach held(tag): closest hit and any hit, nearer
    child first, in a plain scene; closest hit and any hit in stored order in a mirrored one."""
    return (0, 2) if CASES[tag]["mirror"] else (0, 1)


def case(tag):
    """-> (scene, rays (512, 8)) of one name of CASES."""
    c = CASES[tag]
    if tag == "retry":
        return retry(), stack_rays(c["leaves"])
    sc = (instanced if c["family"] == "instanced" else single)(c["S"], c["mirror"])
    return sc, stack_rays(c["leaves"], c["family"] == "instanced")
