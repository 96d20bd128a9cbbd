"""The (base, refit) scene pairs of the vertex-update tests (tests/test_vertex_update_cpu.py, tests/test_gpu_vertex_update.py).

Every case is a base scene and scenes.refit_vertices(base, ...) of it: the scene polaris_hip_update_vertices must make of an uploaded
`base`.  Every deformation is a smooth, seeded function of a vertex's object-space position, so vertices that are
welded in `base` stay welded.  case(name) also says which optional arguments the update passes (normals, matrices).
"""
import functools

import numpy as np

import instance_update_cases as iu_cases
from polaris_amd import scenes

F32 = np.float32


def mesh_vertex_mask(sc, inst):
    """Which rows of sc.vertices belong to the mesh of instance `inst`."""
    idx, _ = scenes._mesh_tree_nodes(sc, int(sc.mesh_instances["bvh_root"][inst]))
    leaf = idx[sc.bvh_nodes["ldata"][idx] <= 0]
    mask = np.zeros(len(sc.vertices), dtype=bool)
    for f, c in zip(-sc.bvh_nodes["ldata"][leaf].astype(np.int64), sc.bvh_nodes["rdata"][leaf].astype(np.int64)):
        mask[3 * f:3 * (f + c)] = True
    return mask


def wave(p, seed, amp):
    """A smooth displacement field: (n, 3) float64 offsets for the positions p, of magnitude about `amp`."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(p), 3))
    ext = max(float(np.ptp(p, axis=0).max()), 1e-6)
    for k in range(3):
        f, ph = rng.uniform(2.0, 7.0, size=3) / ext, rng.uniform(0, 6.28)
        out[:, k] = amp * np.sin(p.astype(np.float64) @ f + ph)
    return out


def deformed(sc, seed, rel=0.03, mask=None):
    """sc.vertices with the masked rows (None: all) displaced by wave(), `rel` of the rows' extent."""
    v = sc.vertices.copy()
    rows = np.ones(len(v), dtype=bool) if mask is None else mask
    p = v[rows, :3]
    v[rows, :3] = (p.astype(np.float64) + wave(p, seed, rel * float(np.ptp(p, axis=0).max()))).astype(F32)
    return v


def _cornell():
    base = scenes.cornell_box("layered")     # 808 triangles, one instance
    return base, scenes.refit_vertices(base, deformed(base, 1, 0.02)), {}


def _moving():
    base, moved = scenes.moving_instances(0), scenes.moving_instances(1)
    return base, scenes.refit_vertices(base, deformed(base, 2, 0.08, mesh_vertex_mask(base, 1)), moved=moved), {"inv": True}


def _cubes():
    base = scenes.instanced_cubes(2)
    return base, scenes.refit_vertices(base, deformed(base, 3, 0.1, mesh_vertex_mask(base, 1))), {}


def _panel():
    base = iu_cases.panel_light()
    v = base.vertices.copy()
    m = mesh_vertex_mask(base, 1)
    v[m, 0] *= F32(1.75)
    v[m, 2] *= F32(1.25)
    return base, scenes.refit_vertices(base, v), {}


def _sphere(with_normals):
    base = scenes.sphere_scene()
    v = deformed(base, 5, 0.02)
    normals = None
    if with_normals:   # smooth normals of the deformed surface, a function of the position like the displacement
        n = base.normals[:, :3].astype(np.float64) + 0.4 * wave(base.vertices[:, :3], 6, 1.0)
        normals = np.zeros_like(base.normals)
        normals[:, :3] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    return base, scenes.refit_vertices(base, v, normals), {"normals": with_normals}


def _grid():
    base = scenes.unique_stress(64)     # displaced_grid(64) and a light: 8 194 triangles, not tiny, a mesh plan of > 1 024 nodes
    return base, scenes.refit_vertices(base, deformed(base, 7, 0.01)), {}


def _big_leaves():
    mt = scenes.MaterialTable()
    kd, light = mt.diffuse((0.7, 0.5, 0.3)), mt.emissive((8, 8, 7), 1.0)
    mesh = scenes.merge([scenes.uv_sphere((0, 1.0, 0), 1.0, kd, n_lat=20, n_lon=24), scenes.quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4), kd),
                         scenes.quad((-1, 3.5, -1), (1, 3.5, -1), (1, 3.5, 1), (-1, 3.5, 1), light)])
    base = scenes.compile_scene([mesh], [(0, np.eye(4))], mt, max_leaf=20, scene_diffuse=mt.diffuse((0.1, 0.1, 0.15)), name="big-leaves")
    base.set_camera(eye=(0, 1.8, 5.0), look=(0, 0.9, 0), fov=0.75, aspect=1.0)
    return base, scenes.refit_vertices(base, deformed(base, 8, 0.02)), {}


def _collapsed():
    """A height field pressed flat onto y = 0, the zero's sign a function of the position: leaves hold +0 and -0 side by side."""
    mt = scenes.MaterialTable()
    kd, blue, light = mt.diffuse((0.6, 0.6, 0.6)), mt.diffuse((0.2, 0.4, 0.7)), mt.emissive((8, 8, 7), 1.0)
    field = scenes.displaced_grid(6, 6.0, 0.5, kd)
    cube = scenes.box((-0.5, 0.2, -0.5), (0.5, 1.2, 0.5), blue)
    lamp = scenes.quad((-1, 3.0, -1), (1, 3.0, -1), (1, 3.0, 1), (-1, 3.0, 1), light)
    base = scenes.compile_scene([field, cube, lamp], [(0, np.eye(4)), (1, scenes.translation((0.3, 0.0, 0.2))), (2, np.eye(4))], mt,
                                scene_diffuse=mt.diffuse((0.1, 0.1, 0.15)), name="collapsed")
    base.set_camera(eye=(0, 2.5, 6.0), look=(0, 0.3, 0), fov=0.7, aspect=1.0)
    v = base.vertices.copy()
    m = mesh_vertex_mask(base, 0)
    sign = np.sin(9.0 * v[m, 0].astype(np.float64) + 5.0 * v[m, 2].astype(np.float64)) < 0
    v[m, 1] = np.where(sign, F32(-0.0), F32(0.0))
    return base, scenes.refit_vertices(base, v), {}


def _reader_boxes():
    """Instances 1 and 4 keep the scene reader's translation-only boxes, which do not bound them: their cull factors are +inf before
    and after the update."""
    base = iu_cases.with_reader_boxes(scenes.transformed_instances(), [1, 4])
    refit = scenes.refit_vertices(base, deformed(base, 10, 0.06, mesh_vertex_mask(base, 1)))
    refit = iu_cases.with_reader_boxes(refit, [1, 4])
    return base, refit, {}


CASES = {
    "cornell": _cornell,                          # tiny mode, LDS triangle records, tiny_one, root_is_instance
    "moving-and-deformed": _moving,               # vertices and matrices change in one call
    "cubes-shared-mesh": _cubes,                  # every instance of the mesh gets a new extent
    "panel-light": _panel,                        # area and light records follow; the panel is one leaf: a mesh root without a pair record
    "sphere-normals": lambda: _sphere(True),
    "sphere-null-normals": lambda: _sphere(False),
    "grid-64": _grid,
    "big-leaves": _big_leaves,                    # leaves of more than 15 triangles: LeafInfo
    "collapsed": _collapsed,                      # zero-extent boxes, +0 beside -0
    "reader-boxes": _reader_boxes,                # +inf cull factors at the top level survive
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(base, refit, passes) of a case, built once per process and shared: leave them unchanged."""
    return CASES[name]()


def update_args(name):
    """(vertices, boxes, normals, inv, emissives) the case's update passes: None where the case leaves the optional array out."""
    _, refit, passes = case(name)
    vertices, boxes, normals, inv, ems = scenes.vertex_update_args(refit)
    return vertices, boxes, normals if passes.get("normals") else None, inv if passes.get("inv") else None, ems
