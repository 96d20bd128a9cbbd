"""Scenes and rays built so that traversal ORDER decides the answer (TEST INFRASTRUCTURE).

DESIGN.md section 2: the kernels traverse in their own order, and an EXACT tie between two triangle tests goes to the one the
reference tests first (intersect.cl:281, strict `t < best`).  Random scenes meet that rule by accident; these meet it on every ray:

* `lattice`: unit quads on the integer lattice at z = 0 and rays that land on its vertices (six triangles tie), edges and diagonals
  (two tie) with exactly representable t -- and whose x / y run exactly in the planes of box faces (0 * inf = NaN in the slab test:
  the reference drops such hits, tree-dependently, and so must every kernel);
* `doubled`: every triangle present twice, the copy with another material: every hit is a tie;
* `coincident_instances`: ties ACROSS instances -- of one mesh (only the instance index tells the twins apart) and of different
  meshes whose instance boxes differ, so that the top-level tree may visit the higher index first;
* `epsilon_edges`: rays on either side of the strict comparisons t > INTERSECTION_EPSILON and |det| < INTERSECTION_EPSILON, and
  zero-area triangles;
* `shadow_variants`: maxDist exactly at, one ulp below and one ulp above a ray's hit distance (t < maxDist).

Only polaris_amd.scenes and seeded numpy.  Twins carry different materials: a wrong winner is another triangle AND another image.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from polaris_amd import scenes as S  # noqa: E402

F32 = np.float32
FLT_MAX = F32(3.402823466e+38)
EPS = F32(0.00001)   # INTERSECTION_EPSILON as the reference's float literal

LATTICE_DIRS = ((0, 0, -1), (0, 0, 1), (1, 0, -1), (0, -1, -1), (1, 1, -2), (-1, 2, -4), (0.5, 0.25, -1))


def _rays(o, d, max_dist=FLT_MAX):
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    rays = np.zeros((len(o), 8), F32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 3] = o, d, max_dist
    return rays


# ---- lattice -----------------------------------------------------------------------------------------------------------------
def lattice(n=8, max_leaf=4, relief=None):
    """n x n unit quads at z = 0 on the integer lattice, two triangles each (all diagonals the same way: an inner vertex belongs to
    six triangles), materials cycling over four diffuse leaves, one emissive triangle, one identity instance (and an environment
    light, so that a frame of it has shadow rays).

    `relief` (a seed): the lattice's vertices get heights drawn from {0, 1, 2, 3} (from {0, 1} in its left half).  Under the vertical rays every det is +-1 and
    t = 4 -+ height stays exact, so the triangles round a vertex still tie -- but now their leaves' boxes differ in z, a ray enters
    them at different distances, and a near-child-first traversal reaches the lower DFS rank SECOND on many of them (on the flat
    lattice all boxes of a tie are entered at the same distance, and such a traversal falls back to the reference's order)."""
    mt = S.MaterialTable()
    leaves = [mt.diffuse((0.8, 0.2, 0.2)), mt.diffuse((0.2, 0.8, 0.2)), mt.diffuse((0.2, 0.2, 0.8)), mt.diffuse((0.7, 0.7, 0.2))]
    light = mt.emissive((6.0, 5.0, 4.0), 2.0)
    parts = []
    z = np.zeros((n + 1, n + 1))
    if relief is not None:   # rough on the right (0 .. 3), gentle on the left (0 .. 1): also big leaves get boxes of different heights
        z = np.random.default_rng(0x4E11EF + relief).integers(0, 4, (n + 1, n + 1)).astype(np.float64)
        z[:, : n // 2] //= 2
    for y in range(n):
        for x in range(n):
            q = S.quad((x, y, z[y, x]), (x + 1, y, z[y, x + 1]), (x + 1, y + 1, z[y + 1, x + 1]), (x, y + 1, z[y + 1, x]), 0)
            k = 2 * (y * n + x)
            q.mat = np.array([leaves[k % 4], leaves[(k + 1) % 4]])
            parts.append(q)
    mesh = S.merge(parts)
    mesh.mat[2 * ((n // 2) * n + n // 2) + 1] = light
    sc = S.compile_scene([mesh], [(0, np.eye(4))], mt, max_leaf=max_leaf, scene_diffuse=mt.diffuse((0.1, 0.1, 0.15)),
                         scene_emissive=mt.emissive((0.6, 0.7, 0.9), 1.0), name=f"{'lattice' if relief is None else 'relief'}-{n}-{max_leaf}")
    return sc.set_camera(eye=(0.5 * n + 0.25, -0.375 * n, 0.75 * n), look=(0.5 * n, 0.5 * n, 0.0), up=(0, 0, 1), fov=0.9, aspect=64 / 48)


def lattice_rays(n=8):
    """Rays that meet z = 0 at every point of the quarter-integer grid on [-0.5, n + 0.5]^2, in seven directions (not normalised),
    from the planes z = +-4: origins, directions and every t (4, 2 or 1) are exact in float32."""
    g = np.arange(-2, 4 * n + 3) * 0.25
    px, py = np.meshgrid(g, g, indexing="xy")
    p = np.stack([px.ravel(), py.ravel(), np.zeros(px.size)], axis=1)
    out = []
    for d in LATTICE_DIRS:
        d = np.asarray(d, np.float64)
        s = 4.0 / abs(d[2])
        out.append(_rays(p - s * d, np.broadcast_to(d, p.shape)))
    return np.concatenate(out)


# ---- doubled -----------------------------------------------------------------------------------------------------------------
def _one_mesh_of_two(sc):
    """A scene compiled from two meshes under one identity instance each -> the same triangles as ONE instance whose mesh tree is a
    new root over the two mesh trees (left: the first mesh).  The two halves' boxes differ, so a ray may enter the right one first."""
    import dataclasses

    nodes = sc.bvh_nodes
    roots = [int(r) for r in sc.mesh_instances["bvh_root"]]
    assert len(roots) == 2 and roots[0] < roots[1] and np.array_equal(sc.mesh_instances["inv_transform"][0], sc.mesh_instances["inv_transform"][1])
    shift = 2 - roots[0]                                   # node 0: the top tree's one leaf; node 1: the new mesh root
    mesh = nodes[roots[0]:].copy()
    inner = mesh["ldata"] > 0
    mesh["ldata"][inner] += shift
    mesh["rdata"][inner] += shift
    head = np.zeros(2, nodes.dtype)
    head["min"], head["max"] = nodes[0]["min"], nodes[0]["max"]
    head[0]["ldata"], head[0]["rdata"] = 0, 0              # top leaf: instance 0
    head[1]["ldata"], head[1]["rdata"] = roots[0] + shift, roots[1] + shift
    inst = sc.mesh_instances[:1].copy()
    inst["bvh_root"] = 1
    return dataclasses.replace(sc, bvh_nodes=np.concatenate([head, mesh]), mesh_instances=inst, bvh_max_depth=sc.bvh_max_depth + 1)


def doubled(max_leaf=4, seed=0, split=False):
    """A flat-shaded uv_sphere(6, 8) and a box round it (92 triangles), every triangle present twice, the copy with another material
    (the sphere's copy is the light), the 184 permuted by `seed`.

    compile_scene's builder keeps twins together (equal centroids): they meet in one leaf or as siblings with equal boxes, where any
    sensible traversal order is the reference's.  `split`: the sphere's first copies get a tree of their own, all the rest another,
    joined under a new root (_one_mesh_of_two, the sphere's tree on the left).  A ray from inside the room is inside the right box
    and reaches the sphere's box later: a near-child-first traversal meets the higher-ranked twin of every sphere hit FIRST."""
    mt = S.MaterialTable()
    a, b = mt.diffuse((0.8, 0.3, 0.2)), mt.emissive((1.0, 0.95, 0.9), 1.5)
    wall, wall2 = mt.diffuse((0.7, 0.7, 0.7)), mt.conductor((0.3, 0.9, 0.4))
    sphere = S.uv_sphere((0.1, -0.2, 0.05), 1.0, a, n_lat=6, n_lon=8, smooth=False)
    room = S.box((2, 2, 2), (-2, -2, -2), wall)   # (corners swapped: the faces look inwards)
    first = S.merge([sphere, room])
    twin = S.merge([sphere, room])
    twin.mat = np.where(first.mat == a, b, wall2)
    both = S.merge([first, twin])
    perm = np.random.default_rng(0xD0B1ED + seed).permutation(len(both.mat))
    mesh = S.Mesh(both.verts[perm], both.normals[perm], both.uvs[perm], both.mat[perm])
    assert len(mesh.mat) == 184
    if split:
        n_sphere = len(sphere.mat)
        halves = [S.Mesh(both.verts[k], both.normals[k], both.uvs[k], both.mat[k]) for k in (perm[perm < n_sphere], perm[perm >= n_sphere])]
        sc = _one_mesh_of_two(S.compile_scene(halves, [(0, np.eye(4)), (1, np.eye(4))], mt, max_leaf=max_leaf, name=f"doubled-split-{max_leaf}-{seed}"))
    else:
        sc = S.compile_scene([mesh], [(0, np.eye(4))], mt, max_leaf=max_leaf, name=f"doubled-{max_leaf}-{seed}")
    return sc.set_camera(eye=(1.6, 0.9, 1.7), look=(0.0, -0.2, 0.0), fov=0.9, aspect=64 / 48)


def doubled_rays(n=20000, seed=1):
    """Random rays from points of [-2.5, 2.5]^3 towards points of it; a tenth with a short maxDist."""
    rng = np.random.default_rng(0xD0B1E + seed)
    o = rng.uniform(-2.5, 2.5, (n, 3)).astype(F32)
    tgt = rng.uniform(-2.5, 2.5, (n, 3)).astype(F32)
    d = (tgt - o).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = _rays(o, d)
    short = rng.random(n) < 0.1
    rays[short, 3] = rng.uniform(0.5, 5.0, int(short.sum())).astype(F32)
    return rays


# ---- coincident instances ----------------------------------------------------------------------------------------------------
ORDERS = ((0, 1, 2), (2, 1, 0), (1, 2, 0), (0, 2, 1))


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def coincident_instances(order=(0, 1, 2), max_leaf=2):
    """Instances 0-2: three DIFFERENT meshes with the same twelve cube triangles -- the cube, and two with the triangles in reversed
    order plus one far outrigger triangle at (-4, 0, 0) / (4, 0, 0), so their instance boxes differ -- at one transform, mesh
    order[k] as instance k.  Instances 3-4 and 5-7: the cube mesh two and three times at one rotated, non-uniformly scaled transform
    each.  Instance 8: a ground quad (and a light over it as instance 9)."""
    mt = S.MaterialTable()
    tints = [mt.diffuse((0.8, 0.2, 0.2)), mt.diffuse((0.2, 0.8, 0.2)), mt.diffuse((0.2, 0.2, 0.8))]
    cube = S.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), tints[0])

    def reversed_with_outrigger(x, mat):
        c = S.Mesh(cube.verts[::-1].copy(), cube.normals[::-1].copy(), cube.uvs[::-1].copy(), np.full(12, mat))
        v = np.array([[[x, 0.0, 0.0], [x, 0.125, 0.0], [x, 0.0, 0.125]]])
        return S.merge([c, S.Mesh(v, S._flat_normals(v), np.zeros((1, 3, 2)), np.array([mat]))])

    ground = S.quad((-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8), mt.diffuse((0.6, 0.6, 0.6)))
    lamp = S.quad((-2, 6, -2), (2, 6, -2), (2, 6, 2), (-2, 6, 2), mt.emissive((5.0, 5.0, 5.0), 2.0))
    meshes = [cube, reversed_with_outrigger(-4.0, tints[1]), reversed_with_outrigger(4.0, tints[2]), ground, lamp]
    x_diff = S.translation((0.0, 1.25, 0.0)) @ _rot(1, 0.4) @ S.scaling(1.0, 1.5, 0.75)
    x_two = S.translation((-2.5, 1.0, 1.0)) @ _rot(1, 0.7) @ _rot(0, 0.3) @ S.scaling(1.25, 0.75, 1.0)
    x_three = S.translation((2.5, 1.5, -1.0)) @ _rot(2, -0.5) @ _rot(1, 1.1) @ S.scaling(0.75, 1.5, 1.25)
    insts = [(int(m), x_diff) for m in order] + [(0, x_two)] * 2 + [(0, x_three)] * 3 + [(3, np.eye(4)), (4, np.eye(4))]
    sc = S.compile_scene(meshes, insts, mt, max_leaf=max_leaf, scene_diffuse=mt.diffuse((0.1, 0.12, 0.2)), name="coincident-" + "".join(map(str, order)))
    return sc.set_camera(eye=(0.25, 2.5, 5.0), look=(0.0, 1.2, 0.0), fov=1.1, aspect=64 / 48)


DIFFERENT_MESH_TWINS, SAME_MESH_TWINS = (0, 1, 2), ((3, 4), (5, 6, 7))
TWIN_CENTRES = ((0.0, 1.25, 0.0), (-2.5, 1.0, 1.0), (2.5, 1.5, -1.0))


def coincident_rays(n=20000, seed=2):
    """Random rays from [-6, 6] x [0, 6] x [-6, 6] towards points near the three groups of twins."""
    rng = np.random.default_rng(0xC01C + seed)
    o = (rng.uniform(-6.0, 6.0, (n, 3)) * (1, 0.5, 1) + (0, 3.0, 0)).astype(F32)
    tgt = (np.asarray(TWIN_CENTRES)[rng.integers(0, 3, n)] + rng.uniform(-0.9, 0.9, (n, 3))).astype(F32)
    d = (tgt - o).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rays(o, d)


# ---- epsilon edges -----------------------------------------------------------------------------------------------------------
def epsilon_edges(max_leaf=4):
    """Four triangles at z = 0: (0,0) (2,0) (0,2) twice (the copy with another material) and two of zero area (collinear vertices;
    two equal vertices) inside it."""
    mt = S.MaterialTable()
    a, b, z = mt.diffuse((0.8, 0.2, 0.2)), mt.diffuse((0.2, 0.8, 0.2)), mt.emissive((1.0, 1.0, 1.0), 1.0)
    v = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]],
                  [[0.125, 0.125, 0], [0.5, 0.5, 0], [0.875, 0.875, 0]],
                  [[0, 0, 0], [2, 0, 0], [0, 2, 0]],
                  [[0.25, 0.25, 0], [0.25, 0.25, 0], [1, 0.5, 0]]], np.float64)
    nrm = np.broadcast_to(np.array([0.0, 0.0, 1.0]), v.shape).copy()
    mesh = S.Mesh(v, nrm, np.zeros((4, 3, 2)), np.array([a, z, b, z]))
    sc = S.compile_scene([mesh], [(0, np.eye(4))], mt, max_leaf=max_leaf, scene_diffuse=mt.diffuse((0.1, 0.1, 0.1)), name=f"epsilon-{max_leaf}")
    return sc.set_camera(eye=(0.5, 0.5, 3.0), look=(0.5, 0.5, 0.0), fov=0.8, aspect=1.0)


def zero_area_triangles(sc):
    """Scene triangle indices whose float32 vertices span no area."""
    v = sc.vertices[:, :3].reshape(-1, 3, 3).astype(np.float64)
    return np.nonzero(np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0)[0]


def _steps():
    """1e-5f * (1 + k * 2^-20), k = -200 .. 199, in float32."""
    k = np.arange(-200, 200)
    return (EPS * (F32(1.0) + (k * 2.0 ** -20).astype(F32))).astype(F32), k


def epsilon_t_rays():
    """400 rays straight down onto (0.25, 0.25, 0) from z = 1e-5f * (1 + k * 2^-20): t == z exactly (det = 4, u = v = 0.125), a hit
    iff t > INTERSECTION_EPSILON, i.e. k > 0."""
    z, k = _steps()
    o = np.stack([np.full(400, 0.25, F32), np.full(400, 0.25, F32), z], axis=1)
    return _rays(o, np.broadcast_to(np.array([0, 0, -1], F32), o.shape)), k


def epsilon_det_rays():
    """400 grazing rays along (1, 0, dz), dz = -(1e-5f / 4) * (1 + k * 2^-20): det = -4 dz exactly, tested iff |det| >= 1e-5f,
    i.e. k >= 0; they meet z = 0 near (0.5, 0.5) at t ~ 1.5."""
    e, k = _steps()
    dz = (-(e * F32(0.25))).astype(F32)
    o = np.stack([np.full(400, -1.0, F32), np.full(400, 0.5, F32), (F32(-1.5) * dz).astype(F32)], axis=1)
    d = np.stack([np.ones(400, F32), np.zeros(400, F32), dz], axis=1)
    return _rays(o, d), k


# ---- shadow variants ---------------------------------------------------------------------------------------------------------
def shadow_variants(rays, hit, t):
    """The hit rays of a set with maxDist == t, one ulp below and one ulp above: {"at", "below", "above"} -> (m, 8) rays."""
    h = np.asarray(hit) != 0
    t = np.asarray(t, F32)[h]
    out = {}
    for name, md in (("at", t), ("below", np.nextafter(t, F32(0))), ("above", np.nextafter(t, F32(np.inf)))):
        r = np.asarray(rays, F32)[h].copy()
        r[:, 3] = md
        out[name] = r
    return out


# ---- independent statements (CPU tests) --------------------------------------------------------------------------------------
def brute_force(sc, rays):
    """Float32 Moeller-Trumbore of EVERY triangle of an identity-instance scene, in array order with the reference's strict
    comparisons, operation for operation (no fused multiply-add: numpy float32).  -> (t (n,) float32 with maxDist where nothing
    was hit, winner (n,) int, multiplicity (n,): how many triangles were accepted at exactly the winning t)."""
    v = sc.vertices[:, :3].reshape(-1, 3, 3)
    o, d, md = rays[:, 0:3].astype(F32), rays[:, 4:7].astype(F32), rays[:, 3].astype(F32)
    n = len(rays)
    best, win, mult = md.copy(), np.full(n, -1, np.int64), np.zeros(n, np.int64)

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    with np.errstate(all="ignore"):
        for k in range(len(v)):
            v0 = np.broadcast_to(v[k, 0], o.shape)
            e1, e2 = np.broadcast_to(v[k, 1] - v[k, 0], o.shape), np.broadcast_to(v[k, 2] - v[k, 0], o.shape)
            p = cross(d, e2)
            det = dot(e1, p)
            inv = F32(1.0) / det
            tv = o - v0
            u = dot(tv, p) * inv
            q = cross(tv, e1)
            w = dot(d, q) * inv
            t = dot(e2, q) * inv
            ok = (np.abs(det) >= EPS) & (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1) & (t > EPS) & (t < md)
            mult = np.where(ok & (t == best) & (win >= 0), mult + 1, mult)
            better = ok & (t < best)
            best, win, mult = np.where(better, t, best), np.where(better, k, win), np.where(better, 1, mult)
    return best, win, mult


def dfs_triangle_order(sc, root=None):
    """Scene triangle indices in the order a left-first depth-first walk of a mesh tree of sc.bvh_nodes reaches them."""
    nodes = sc.bvh_nodes
    root = int(sc.mesh_instances[0]["bvh_root"]) if root is None else root
    out, stack = [], [root]
    while stack:
        nd = nodes[stack.pop()]
        if int(nd["ldata"]) <= 0:
            out.extend(range(-int(nd["ldata"]), -int(nd["ldata"]) + int(nd["rdata"])))
        else:
            stack.append(int(nd["rdata"]))
            stack.append(int(nd["ldata"]))
    return np.asarray(out, np.int64)


def dfs_instance_order(sc):
    """Instance indices in the order a left-first depth-first walk of the top tree reaches them."""
    nodes = sc.bvh_nodes
    out, stack = [], [0]
    while stack:
        nd = nodes[stack.pop()]
        if int(nd["ldata"]) <= 0:
            out.append(-int(nd["ldata"]))
        else:
            stack.append(int(nd["rdata"]))
            stack.append(int(nd["ldata"]))
    return out


def twin_of(sc):
    """For a scene whose every triangle is present twice: twin[i] = the scene index of triangle i's copy."""
    v = np.ascontiguousarray(sc.vertices[:, :3].reshape(-1, 9))
    key = {}
    twin = np.full(len(v), -1, np.int64)
    for i, row in enumerate(v):
        j = key.setdefault(row.tobytes(), i)
        if j != i:
            twin[i], twin[j] = j, i
    return twin


# ---- the cases the CPU and GPU tests share -----------------------------------------------------------------------------------
LATTICE_LEAVES = (1, 2, 4, 10)
RELIEF_LEAVES = (1, 4, 20)
DOUBLED = ((1, 0), (2, 1), (4, 2), (10, 3))   # (max_leaf, seed)
DOUBLED_SPLIT = ((1, 4), (4, 5))
EPSILON_LEAVES = (1, 2, 4)

CASES = ([f"lattice-{m}" for m in LATTICE_LEAVES] + ["lattice-big-leaf", "lattice-40"] + [f"relief-{m}" for m in RELIEF_LEAVES] + [f"doubled-{m}-{s}" for m, s in DOUBLED] + [f"doubled-split-{m}-{s}" for m, s in DOUBLED_SPLIT]
         + ["coincident-" + "".join(map(str, o)) for o in ORDERS] + [f"epsilon-{m}" for m in EPSILON_LEAVES])
FAMILIES = {f: [c for c in CASES if c.startswith(f)] for f in ("lattice", "relief", "doubled", "coincident", "epsilon")}


def case(tag):
    """-> (scene, rays (n <= 40 000, 8)) of one name of CASES.  lattice-big-leaf: leaves of 20 triangles (the kernels' big-leaf loop of
    more than 15); lattice-40: 40 x 40 quads, 3 200 triangles (more slots than the tiny-scene modes take), every fifth ray of its
    grid."""
    kind, _, arg = tag.partition("-")
    if tag == "lattice-big-leaf":
        return lattice(8, 20), lattice_rays(8)
    if tag == "lattice-40":
        return lattice(40, 4), lattice_rays(40)[::5].copy()
    if kind == "lattice":
        return lattice(8, int(arg)), lattice_rays(8)
    if kind == "relief":   # (relief-20: big leaves again)
        return lattice(8, int(arg), relief=int(arg)), lattice_rays(8)
    if kind == "doubled":
        m, s = (int(v) for v in arg.replace("split-", "").split("-"))
        return doubled(m, s, split="split" in arg), doubled_rays()
    if kind == "coincident":
        return coincident_instances(tuple(int(c) for c in arg)), coincident_rays()
    if kind == "epsilon":
        return epsilon_edges(int(arg)), np.concatenate([epsilon_t_rays()[0], epsilon_det_rays()[0]])
    raise KeyError(tag)
