"""The (base, moved) scene pairs of the instance-update tests (tests/test_instance_update_cpu.py, tests/test_gpu_instance_update.py).

Every case is a base scene and the same scene with its instances somewhere else; `moved` is compiled afresh, so its top-level
tree may differ from base's in topology -- scenes.refit_instances(base, moved) is what an update of an uploaded `base` must equal.
"""
import functools

import numpy as np

from polaris_amd import scenes

F32 = np.float32


def with_reader_boxes(sc, which):
    """`sc` with the top-level leaf boxes of the instances `which` replaced by the reference scene reader's: the mesh's box moved by
    the translation alone (asset/scene/reader/wavefront.go:514-519) -- under a rotation or a scale it does not bound its instance."""
    boxes = scenes.instance_boxes(sc)
    for i in which:
        mi = sc.mesh_instances[i]
        t = np.linalg.inv(mi["inv_transform"].reshape(4, 4).T.astype(np.float64))[:3, 3].astype(F32)
        root = sc.bvh_nodes[mi["bvh_root"]]
        boxes[i, :3], boxes[i, 3:] = root["min"] + t, root["max"] + t
    out = scenes.refit_instances(sc, sc)
    idx, _ = scenes._top_level_nodes(out)
    leaf = idx[out.bvh_nodes["ldata"][idx] <= 0]
    inst = -out.bvh_nodes["ldata"][leaf].astype(np.int64)
    out.bvh_nodes["min"][leaf], out.bvh_nodes["max"][leaf] = boxes[inst, :3], boxes[inst, 3:]
    out = scenes.refit_instances(out, out)   # the inner nodes follow their leaves
    out.name = sc.name + "-reader-boxes"
    return out


def singular(sc, i):
    """`sc` with instance i's inverse matrix made singular (its third column zero): finite, but not invertible."""
    out = scenes.refit_instances(sc, sc)
    m = out.mesh_instances["inv_transform"][i].copy()
    m[8:12] = 0.0
    out.mesh_instances["inv_transform"][i] = m
    out.name = sc.name + "-singular"
    return out


def translated(sc, seed):
    """`sc` with every instance but the first (the room) translated by a seeded random offset: matrices and leaf boxes follow."""
    rng = np.random.default_rng(seed)
    out = scenes.refit_instances(sc, sc)
    boxes = scenes.instance_boxes(sc)
    for i in range(1, len(sc.mesh_instances)):
        off = rng.uniform(-0.4, 0.4, size=3) * (1.0, 0.25, 1.0)
        fwd = scenes.translation(off) @ np.linalg.inv(sc.mesh_instances["inv_transform"][i].reshape(4, 4).T.astype(np.float64))
        out.mesh_instances["inv_transform"][i] = np.linalg.inv(fwd).T.reshape(-1).astype(F32)
        boxes[i, :3] += off.astype(F32)
        boxes[i, 3:] += off.astype(F32)
    idx, _ = scenes._top_level_nodes(out)
    leaf = idx[out.bvh_nodes["ldata"][idx] <= 0]
    inst = -out.bvh_nodes["ldata"][leaf].astype(np.int64)
    out.bvh_nodes["min"][leaf], out.bvh_nodes["max"][leaf] = boxes[inst, :3], boxes[inst, 3:]
    out = scenes.refit_instances(out, out)
    out.name = sc.name + "-translated"
    return out


def _cubes(n_side):
    base = scenes.instanced_cubes(n_side)
    return base, translated(base, seed=n_side)


def panel_light(turn=0.0):
    """A light panel that turns and stretches about the origin, over a floor and between two cubes.  The reference takes an area
    light's sample points through the INVERSE instance matrix (quirk a-9(4)): transformed_instances' panel, 3.5 above its ground,
    samples 3.5 BELOW it, where every shadow ray is occluded -- its emissive transform cannot be seen in a frame.  Here the matrix
    has no translation, so the sample points stay in the panel's plane and the floor sees them."""
    mt = scenes.MaterialTable()
    grey, blue = mt.diffuse((0.6, 0.6, 0.6)), mt.diffuse((0.2, 0.4, 0.7))
    light = mt.emissive((6, 6, 5), 1.5)
    panel = scenes.merge([scenes.quad((-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5), light)])
    floor = scenes.quad((-5, -1.5, -5), (-5, -1.5, 5), (5, -1.5, 5), (5, -1.5, -5), grey)
    cube = scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), blue)
    insts = [(1, np.eye(4)), (0, scenes.rotation_y(0.3 + turn) @ scenes.scaling(2.0 + 2.0 * turn, 1.0, 1.0)),
             (2, scenes.translation((-2.0, -1.0, 0.5))), (2, scenes.translation((2.2, -1.0 + 0.3 * turn, -0.4)) @ scenes.rotation_y(turn))]
    sc = scenes.compile_scene([panel, floor, cube], insts, mt, scene_diffuse=mt.diffuse((0.05, 0.05, 0.08)), name=f"panel-light-{turn}")
    sc.set_camera(eye=(0, 1.5, 7.0), look=(0, -0.8, 0), fov=0.75, aspect=1.0)
    return sc


def _transformed():
    # boxes that do not bound and factors of +inf flip in BOTH directions: instance 1 (the turned cube) goes from the reader's box to
    # an exact one, instance 2 the other way; instance 4 keeps the reader's box
    return with_reader_boxes(scenes.transformed_instances(), [1, 4]), with_reader_boxes(scenes.transformed_instances(turn=0.7), [2, 4])


def _swarm17_singular():
    return scenes.instance_swarm(17, seed=5), singular(scenes.instance_swarm(17, seed=5, step=2), 6)


def _cornell_one():
    w = scenes.translation((0.05, 0.0, -0.02)) @ scenes.rotation_y(0.1)
    return scenes.cornell_box("diffuse"), scenes.cornell_box("diffuse", world=w)


CASES = {
    "moving-0-1": lambda: (scenes.moving_instances(0), scenes.moving_instances(1)),
    "moving-0-8": lambda: (scenes.moving_instances(0), scenes.moving_instances(8)),
    "transformed-returned": _transformed,
    "panel-light": lambda: (panel_light(), panel_light(0.8)),
    "one-instance": _cornell_one,                       # root_is_instance: no top-level pair record
    "cubes-1": lambda: _cubes(1),
    "cubes-2": lambda: _cubes(2),                       # instances sharing a mesh
    "cubes-3": lambda: _cubes(3),
    "swarm-17": lambda: (scenes.instance_swarm(17, seed=5), scenes.instance_swarm(17, seed=5, step=3)),  # NI > 16: the renumbering stays out of the meshes
    "swarm-150": lambda: (scenes.instance_swarm(150, seed=11), scenes.instance_swarm(150, seed=11, step=4)),
    "swarm-17-singular": _swarm17_singular,
    "swarm-600": lambda: (scenes.instance_swarm(600, seed=2), scenes.instance_swarm(600, seed=2, step=1)),  # a plan too big for one workgroup: a launch per level
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(base, moved, refit) of a case, built once per process and shared: leave them unchanged."""
    base, moved = CASES[name]()
    return base, moved, scenes.refit_instances(base, moved)
