"""An independent numpy statement of the temporal reprojection across mesh deformation (option "vertex_motion", DESIGN.md section
10k), a small ray caster over instanced triangles that makes engineered planes for it, the two-instance Cornell box whose tall block
the tests deform, and the quality run that scripts/vertex_motion_quality.py tabulates and tests/test_vertex_motion_cpu.py guards.

The statement is written from the algorithm's text with whole-frame float64 arrays: a pixel whose triangle has the same 36 bytes of
xyz now and in the history's vertices goes through D_k = inverse(Inv_hist[k]) . Inv_cur[k] as motion_oracle states it; any other
starts from the point of the OLD triangle at the hit's barycentrics, taken to the history's world through np.linalg.inv(Inv_hist[k]).
The projection is np.linalg.solve, the taps fancy indexing.  It shares no code with polaris_amd/csrc/temporal.h, which the kernels
and polaris_host_reproject_deform include.
"""
from __future__ import annotations

import numpy as np

import motion_oracle as MO
import temporal_oracle as TO
from gbuffer_oracle import FLT_MAX, filtered_mask, leaf_word
from polaris_amd import ctypes_api as T

F = np.float32
NO_TRIANGLE = np.uint32(0xFFFFFFFF)
IDENTITY16 = np.eye(4, dtype=F).reshape(-1)


def hit_plane(tri, u, v) -> np.ndarray:
    """The (H, W, 4) uint32 HIT plane of (H, W) triangle indices (< 0: a miss) and float32 barycentrics."""
    tri = np.asarray(tri, np.int64)
    out = np.zeros(tri.shape + (4,), np.uint32)
    out[..., 0] = np.where(tri < 0, int(NO_TRIANGLE), tri).astype(np.uint32)
    out[..., 1] = np.where(tri < 0, 0, np.ascontiguousarray(u, F).view(np.uint32))
    out[..., 2] = np.where(tri < 0, 0, np.ascontiguousarray(v, F).view(np.uint32))
    return out


def changed_triangles(vertices, prev_vertices) -> np.ndarray:
    """(NT,) bool: the 36 bytes of the triangle's xyz differ between the two (3 NT, 4) arrays."""
    a = np.ascontiguousarray(np.asarray(vertices, F).reshape(-1, 3, 4)[:, :, :3]).view(np.uint32).reshape(-1, 9)
    b = np.ascontiguousarray(np.asarray(prev_vertices, F).reshape(-1, 3, 4)[:, :, :3]).view(np.uint32).reshape(-1, 9)
    return np.any(a != b, axis=1)


def reproject_deform(history, prev_guide, prev_albedo, prev_inst, prev_eye, prev_frustum, guide, albedo, inst, eye, frustum, prev_inv, inv,
                     hit, vertices, prev_vertices, *, max_history=32, normal_threshold=0.9, depth_threshold=0.1, history_variance=None,
                     position_margin=True):
    """(prior (H, W, 4) float64, margin (H, W) float64), or (prior, prior2, margin) with the history's VARIANCE plane, as
    motion_oracle.reproject_motion states them; the point that is projected into the history camera is the deformation's."""
    H, W = guide.shape[:2]
    prior = np.zeros((H, W, 4))
    prior2 = np.zeros((H, W, 4))
    margin = np.full((H, W), np.inf)
    done = lambda: (prior, margin) if history_variance is None else (prior, prior2, margin)  # noqa: E731
    if not TO.projectable(prev_frustum) or max_history == 0:
        return done()
    prev_inv, inv = np.asarray(prev_inv, F).reshape(-1, 16), np.asarray(inv, F).reshape(-1, 16)
    n_inst = len(inv)
    cur_v = np.asarray(vertices, F).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    old_v = np.asarray(prev_vertices, F).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    NT = len(cur_v)
    changed = changed_triangles(vertices, prev_vertices)
    inst = np.asarray(inst, np.uint32)
    prev_inst = np.asarray(prev_inst, np.uint32)
    hit = np.asarray(hit, np.uint32)
    tri = hit[..., 0]
    filt = filtered_mask(albedo) & (inst < n_inst) & (tri < NT)
    ys, xs = np.nonzero(filt)
    if len(ys) == 0:
        return done()
    k_i = inst[ys, xs].astype(np.int64)
    t_i = tri[ys, xs].astype(np.int64)
    # the rigid part: D_k on the first hit
    flags = np.zeros(n_inst, np.int64)
    Ds = np.zeros((n_inst, 3, 4))
    mflags = np.zeros(n_inst, np.int64)
    Ms = np.zeros((n_inst, 3, 4))
    for k in range(n_inst):
        flags[k], Ds[k] = MO.motion(prev_inv[k], inv[k])
        mflags[k], Ms[k] = MO.motion(prev_inv[k], IDENTITY16)          # inverse(Inv_hist[k]): mesh space -> the history's world
    d = TO.centre_dirs(eye, frustum, W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(eye, np.float64) + guide[..., 3].astype(np.float64)[..., None] * d
    ps = p[ys, xs]
    ps = np.einsum("nij,nj->ni", Ds[k_i][:, :, :3], ps) + Ds[k_i][:, :, 3]
    alive = flags[k_i] != MO.INVALID
    # the deformed part: the old triangle's point at the hit's barycentrics, through inverse(Inv_hist[k])
    ch = changed[t_i]
    bu = np.ascontiguousarray(hit[ys, xs, 1]).view(F).astype(np.float64)
    bv = np.ascontiguousarray(hit[ys, xs, 2]).view(F).astype(np.float64)
    bw = 1.0 - (bu + bv)
    with np.errstate(invalid="ignore", over="ignore"):
        q = bw[:, None] * old_v[t_i, 0] + bu[:, None] * old_v[t_i, 1] + bv[:, None] * old_v[t_i, 2]
        pq = np.einsum("nij,nj->ni", Ms[k_i][:, :, :3], np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0)) + Ms[k_i][:, :, 3]
        finite = np.all(np.isfinite(q.astype(F)), axis=1) & np.all(np.isfinite(pq.astype(F)), axis=1)
    ps = np.where(ch[:, None], pq, ps)
    alive = np.where(ch, (mflags[k_i] != MO.INVALID) & finite, alive)
    ys, xs, k_i, ps = ys[alive], xs[alive], k_i[alive], ps[alive]
    if len(ys) == 0:
        return done()
    fr = np.asarray(prev_frustum, np.float64).reshape(4, 4)[:, :3]
    tl, tr, bl = fr[0], fr[1], fr[2]
    qs = ps - np.asarray(prev_eye, np.float64)
    M = np.empty((len(ys), 3, 3))
    M[:, :, 0] = tr - tl
    M[:, :, 1] = bl - tl
    M[:, :, 2] = -qs
    sol = np.linalg.solve(M, np.broadcast_to(-tl, (len(ys), 3))[..., None])[..., 0]
    u, v, mu = sol[:, 0], sol[:, 1], sol[:, 2]
    dist = np.linalg.norm(qs, axis=-1)
    x, y = u * W - 0.5, v * H - 0.5
    mg = np.abs(mu) / (1 + np.abs(mu))
    ok = (mu > 0) & (x > -1) & (x < W) & (y > -1) & (y < H)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    if position_margin:
        mg = np.minimum(mg, np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)))
    n_i = guide[ys, xs, :3].astype(np.float64)
    leaf_i = np.ascontiguousarray(albedo[ys, xs, 3]).view(np.uint32)
    hleaf = np.ascontiguousarray(prev_albedo[..., 3]).view(np.uint32)
    sw = np.zeros(len(ys))
    acc = np.zeros((len(ys), 4))
    acc2 = np.zeros(len(ys))
    for k in range(4):
        xx = np.where(ok, x0, 0).astype(np.int64) + (k & 1)
        yy = np.where(ok, y0, 0).astype(np.int64) + (k >> 1)
        w = (fx if k & 1 else 1 - fx) * (fy if k >> 1 else 1 - fy)
        inside = ok & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
        c = history[yc, xc].astype(np.float64)
        g = prev_guide[yc, xc].astype(np.float64)
        dot = np.sum(n_i * g[:, :3], axis=-1)
        with np.errstate(invalid="ignore"):
            dz = np.abs(g[:, 3] - dist) - depth_threshold * dist
        near = inside & (c[:, 3] > 0) & np.all(np.isfinite(c[:, :3]), axis=-1) & (hleaf[yc, xc] == leaf_i) & (prev_inst[yc, xc] == k_i)
        valid = near & (dot >= normal_threshold) & (dz <= 0)
        mg = np.where(near, np.minimum(mg, np.minimum(np.abs(dot - normal_threshold), np.abs(np.nan_to_num(dz, nan=1.0)) / np.maximum(dist, 1e-30))), mg)
        sw += np.where(valid, w, 0)
        acc += np.where(valid[:, None], w[:, None] * np.where(valid[:, None], c, 0), 0)
        if history_variance is not None:
            acc2 += np.where(valid, w * history_variance[yc, xc, 1].astype(np.float64), 0)
    has = sw > 0
    out = np.zeros((len(ys), 4))
    out[has] = acc[has] / sw[has, None]
    out[has, 3] = np.minimum(out[has, 3], max_history)
    has &= out[:, 3] > 0
    out[~has] = 0
    prior[ys, xs] = out
    out2 = np.zeros((len(ys), 4))
    out2[has, 0] = acc2[has] / sw[has]
    out2[has, 3] = out[has, 3]
    prior2[ys, xs] = out2
    margin[ys, xs] = mg
    return done()


# ---- a ray caster over instanced triangles -------------------------------------------------------------------------------------
def cast(eye, frustum, W, H, vertices, tri_inst, tri_leaf, worlds):
    """(guide, albedo, INSTANCE, HIT) of a camera over the triangles of `vertices` ((3 NT, 4), mesh space): triangle T belongs to
    instance tri_inst[T] (world matrix worlds[k]) and shows the leaf type tri_leaf[T].  As on the device the ray goes to mesh space
    through the inverse matrix with its direction not renormalised (t is the world distance), the guide normal is the triangle's in
    mesh space, turned towards the ray, and u, v weigh the second and third vertex."""
    dirs = TO.centre_dirs(eye, frustum, W, H).reshape(-1, 3)
    e = np.asarray(eye, np.float64)
    n_px = len(dirs)
    best = np.full(n_px, np.inf)
    guide = np.zeros((n_px, 4), F)
    guide[:, 3] = FLT_MAX
    albedo = np.ones((n_px, 4), F)
    albedo[:, 3] = leaf_word(np.full(n_px, -1))
    inst = np.full(n_px, MO.NO_INSTANCE, np.uint32)
    tri, bu, bv = np.full(n_px, -1, np.int64), np.zeros(n_px, F), np.zeros(n_px, F)
    v = np.asarray(vertices, F).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    for t_idx in range(len(v)):
        k = int(tri_inst[t_idx])
        inv = np.linalg.inv(np.asarray(worlds[k], np.float64))
        o = inv[:3, :3] @ e + inv[:3, 3]
        dm = dirs @ inv[:3, :3].T
        a, b, c = v[t_idx]
        e1, e2 = b - a, c - a
        pv = np.cross(dm, e2)
        det = pv @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            tv = o - a
            uu = (pv @ tv) / det
            qv = np.cross(tv, e1)
            vv = (dm @ qv) / det
            tt = (qv @ e2) / det
        hit = (np.abs(det) > 1e-12) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 1e-6) & (tt < best)
        n = np.cross(e1, e2)
        n = n / np.linalg.norm(n)
        best = np.where(hit, tt, best)
        guide[hit, :3] = np.where(((dm[hit] @ n) < 0)[:, None], n, -n).astype(F)
        guide[hit, 3] = tt[hit].astype(F)
        albedo[hit, :3] = F(0.5)
        albedo[hit, 3] = leaf_word(np.full(int(hit.sum()), int(tri_leaf[t_idx])))
        inst[hit] = k
        tri[hit], bu[hit], bv[hit] = t_idx, uu[hit].astype(F), vv[hit].astype(F)
    sh = (H, W)
    return guide.reshape(H, W, 4), albedo.reshape(H, W, 4), inst.reshape(sh), hit_plane(tri.reshape(sh), bu.reshape(sh), bv.reshape(sh))


def quad_tris(x0, x1, y0, y1, z):
    """Two triangles ((6, 4) float32 vertices) of the rectangle [x0, x1] x [y0, y1] at depth z, facing +z."""
    p = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    out = np.zeros((6, 4), F)
    out[:, :3] = np.asarray([p[0], p[1], p[2], p[0], p[2], p[3]], F)
    return out


# ---- engineered cases for the restatement and the kernel ------------------------------------------------------------------------
ORDER = ("hist", "pg", "pa", "pi", "pe", "pf", "g", "a", "i", "e", "f", "pt", "ct", "hit", "v", "pv")
N_INST, N_TRIS = 3, 16


def args(c):
    return [c[k] for k in ORDER]


def engineered_cases(W=32, H=24, seed=0):
    """[(name, dict)]: 16 triangles in 3 instances seen under two cameras -- instance 0 a wall of four quads behind (STATIC), instances
    1 and 2 two quads each in front of it (MOVED) -- with the first quad of every instance deformed between the history and now and
    the others not, a lamp (not filtered) and misses around the wall.  The dict's keys are the arguments of reproject_deform in order
    plus hvar.  Variants put in what the base case cannot show: an INVALID instance (in the current matrix alone, where the changed
    triangles keep their history, and in the history's), words outside the tables, non-finite history vertices, an instance mismatch
    at the taps."""
    import test_temporal_cpu as TC
    from polaris_amd import scenes as S

    rng = np.random.default_rng(5 + 3 * W + seed)
    wall = [quad_tris(-1.4, 0, -1.2, 0, -4.0), quad_tris(0, 1.4, -1.2, 0, -4.0), quad_tris(-1.4, 0, 0, 1.2, -4.0), quad_tris(0, 1.4, 0, 1.2, -4.0)]
    left = [quad_tris(-1.0, -0.2, -0.6, 0.0, -3.0), quad_tris(-1.0, -0.2, 0.0, 0.6, -3.0)]
    right = [quad_tris(0.2, 1.0, -0.6, 0.0, -3.0), quad_tris(0.2, 1.0, 0.0, 0.6, -3.0)]
    old = np.concatenate(wall + left + right)
    assert len(old) == 3 * N_TRIS
    tri_inst = np.array([0] * 8 + [1] * 4 + [2] * 4)
    tri_leaf = np.full(N_TRIS, T.BXDF_DIFFUSE)
    tri_leaf[6:8] = T.BXDF_EMISSIVE                                    # the wall's last quad is a lamp
    new = old.copy()
    for first in (0, 8, 12):                                           # the first quad of every instance: sheared in its plane, bulged a little
        rows = slice(3 * first, 3 * first + 6)
        x, y = old[rows, 0].astype(np.float64), old[rows, 1].astype(np.float64)
        new[rows, 0] = (x + 0.12 * np.sin(2.0 * y + first)).astype(F)
        new[rows, 1] = (y + 0.10 * np.cos(1.5 * x)).astype(F)
        new[rows, 2] = (old[rows, 2] + 0.04 * np.sin(3.0 * x + y)).astype(F)
    pe, pf = TO.pinhole((0, 0, 0))
    e, f = TO.pinhole((0.04, 0.02, 0))
    eye4 = np.eye(4)
    about = lambda m: S.translation((0.6, 0, -3)) @ m @ S.translation((-0.6, 0, 3))  # noqa: E731  (instance 2 stands around there)
    hist_worlds = [eye4, S.translation((0.05, 0.02, 0)), about(S.rotation_y(0.05))]
    cur_worlds = [eye4, S.translation((0.15, -0.03, -0.05)), about(S.rotation_y(0.12) @ S.scaling(1.0, 1.05, 1.0))]

    def case(verts=new, prev=old):
        pg, pa, pi, _ = cast(pe, pf, W, H, prev, tri_inst, tri_leaf, hist_worlds)
        g, a, i, hit = cast(e, f, W, H, verts, tri_inst, tri_leaf, cur_worlds)
        hvar = (rng.random((H, W, 4)) * 2).astype(F)
        return dict(hist=TC.history_planes(rng, H, W), pg=pg, pa=pa, pi=pi, pe=pe, pf=pf, g=g, a=a, i=i, e=e, f=f,
                    pt=np.stack([MO.inv16(w) for w in hist_worlds]), ct=np.stack([MO.inv16(w) for w in cur_worlds]), hit=hit,
                    v=verts.copy(), pv=prev.copy(), hvar=hvar)

    cases = [("deformed", case()), ("undeformed", case(old, old))]
    c = case()
    c["ct"][2, 0:4] = 0                                                # a zero column in instance 2's current inverse matrix:
    cases.append(("invalid now", c))                                   # its unchanged triangles lose their history, the changed ones do not
    c = case()
    c["pt"][2, 4:8] = 0                                                # ... in the history's: neither has any
    cases.append(("invalid then", c))
    c = case()
    r = rng.random((H, W))
    c["hit"][r < 0.06, 0] = N_TRIS                                     # triangle words outside the scene on filtered pixels
    c["hit"][(r >= 0.06) & (r < 0.1), 0] = NO_TRIANGLE
    c["hit"][(r >= 0.1) & (r < 0.13), 0] = 1 << 24
    c["i"][(r >= 0.13) & (r < 0.17)] = N_INST                          # instance words outside the table
    c["i"][(r >= 0.17) & (r < 0.2)] = MO.NO_INSTANCE
    cases.append(("words outside", c))
    c = case()
    c["pv"][3 * 0 + 1, 0] = np.nan                                     # a history vertex of a changed wall triangle, of one of instance 1
    c["pv"][3 * 8 + 2, 2] = np.inf
    cases.append(("non-finite", c))
    c = case()
    blk = (slice(H // 4, H // 2), slice(W // 4, 3 * W // 4))
    c["pi"][blk] = (c["pi"][blk] + 1) % 3                              # the history shows another instance there (misses: instance 0)
    cases.append(("instance mismatch", c))
    return cases


# ---- the two-instance Cornell box -----------------------------------------------------------------------------------------------
def cornell_two_instances(aspect=1.0, mirror=False):
    """The Cornell-diffuse box as two mesh instances: 0 the room with its light and the short block, 1 the tall block (which the
    tests deform).  mirror: the short block is a mirror (for the option "guide_specular").  Camera: cornell_box's."""
    from polaris_amd import scenes as S

    s = 1.0 / 555.0
    mt = S.MaterialTable()
    white, red, green = mt.diffuse((0.725, 0.71, 0.68)), mt.diffuse((0.63, 0.065, 0.05)), mt.diffuse((0.14, 0.45, 0.091))
    light = mt.emissive((17.0, 12.0, 4.0), 1.0)
    short_mat = mt.conductor((0.9, 0.9, 0.95)) if mirror else white
    X, Y, Z = 556.0 * s, 548.8 * s, 559.2 * s
    room = S.merge([
        S.quad((X, 0, 0), (0, 0, 0), (0, 0, Z), (X, 0, Z), white),
        S.quad((X, Y, 0), (X, Y, Z), (0, Y, Z), (0, Y, 0), white),
        S.quad((X, 0, Z), (0, 0, Z), (0, Y, Z), (X, Y, Z), white),
        S.quad((0, 0, Z), (0, 0, 0), (0, Y, 0), (0, Y, Z), green),
        S.quad((X, 0, 0), (X, 0, Z), (X, Y, Z), (X, Y, 0), red),
        S.quad((343 * s, Y - 1e-3, 227 * s), (343 * s, Y - 1e-3, 332 * s), (213 * s, Y - 1e-3, 332 * s), (213 * s, Y - 1e-3, 227 * s), light),
        S.box((130 * s, 0, 65 * s), (130 * s + 165 * s, 165 * s, 65 * s + 165 * s), short_mat, rot_y=0.29),
    ])
    tall = S.box((265 * s, 0, 296 * s), (265 * s + 165 * s, 330 * s, 296 * s + 165 * s), white, rot_y=-0.29)
    sc = S.compile_scene([room, tall], [(0, np.eye(4)), (1, S.translation((0.0, 0.0, 0.02)))], mt, name="cornell-two-instances")
    sc.set_camera(eye=(278 * s, 273 * s, -800 * s), look=(278 * s, 273 * s, 0), fov=0.6911, aspect=aspect)
    return sc


def deformed_block(base, step, rel=0.04):
    """`base` (cornell_two_instances) with the tall block's vertices displaced by tests/vertex_update_cases.deformed, seeded by the step
    (0: base itself), as the scene polaris_hip_update_vertices makes of an uploaded base."""
    import vertex_update_cases as VC
    from polaris_amd import scenes as S

    if step == 0:
        return base
    return S.refit_vertices(base, VC.deformed(base, 40 + step, rel, VC.mesh_vertex_mask(base, 1)))


def gbuffer_hit(oracle, sc, W, H):
    """(guide, albedo, INSTANCE, HIT) of a compiled scene on the CPU oracle."""
    import gbuffer_oracle as G

    guide, albedo, _ = G.gbuffer(oracle, sc, W, H)
    hit, wuvt, it = oracle.intersect(sc, G.centre_rays(sc, W, H))
    hit = np.asarray(hit).reshape(-1) != 0
    it = np.asarray(it)
    inst = np.where(hit, it[:, 0].astype(np.int64), int(MO.NO_INSTANCE)).astype(np.uint32)
    wuvt = np.asarray(wuvt, F)
    plane = hit_plane(np.where(hit, it[:, 1].astype(np.int64), -1).reshape(H, W), wuvt[:, 1].reshape(H, W), wuvt[:, 2].reshape(H, W))
    return guide, albedo, inst.reshape(H, W), plane


# ---- the quality run ---------------------------------------------------------------------------------------------------------
def quality_run(host, oracle, steps, N=128, hist_spp=64, spp=1, ref_spp=1024, report=(1,), params=None, seed=0):
    """The tall block of cornell_two_instances deformed anew at every step k = 1 .. steps, the room static: a history of hist_spp at
    step 0, then spp at every step, three ways -- (a) the history reprojected with vertex motion, (b) no history (an update without
    the option: the plain mean of the step's samples), (c) the history kept but reprojected with object motion's rigid arithmetic
    only.  For every step in `report`: {setting: {pixel set: RMSE}} of the unfiltered TEMPORAL plane against ref_spp at that step,
    over the filtered pixels ("all") and those of the deformed block ("block"); "reused": the share of "block" with m > 0 in (a)."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    params = dict(T.TEMPORAL_DEFAULTS if params is None else params)
    base = cornell_two_instances()
    sc0 = base
    acc0, _, _ = oracle.trace(sc0, ob.make_request(N, N, spp=hist_spp, bounces=5), scenes.make_seeds(hist_spp, 5, base=7 + 1000 * seed))
    g0, a0, i0, _ = gbuffer_hit(oracle, sc0, N, N)
    first = host.temporal_combine(acc0, np.zeros_like(acc0), 0, hist_spp)
    hist = {"a": first, "c": first}
    prev = (sc0, g0, a0, i0)
    out = {}
    for k in range(1, steps + 1):
        sc = deformed_block(base, k)
        acc, _, _ = oracle.trace(sc, ob.make_request(N, N, spp=spp, bounces=5), scenes.make_seeds(spp, 5, base=100 + k + 1000 * seed))
        g, a, i, h = gbuffer_hit(oracle, sc, N, N)
        psc, pg, pa, pi = prev
        inv = MO.inv_table(sc)
        pr_a = host.reproject_deform(hist["a"], pg, pa, pi, psc.eye, psc.frustum, g, a, i, sc.eye, sc.frustum, inv, inv, h, sc.vertices, psc.vertices, **params)
        pr_c = host.reproject_motion(hist["c"], pg, pa, pi, psc.eye, psc.frustum, g, a, i, sc.eye, sc.frustum, inv, inv, **params)
        hist = {"a": host.temporal_combine(acc, pr_a, 0, spp), "c": host.temporal_combine(acc, pr_c, 0, spp)}
        planes = {"a": hist["a"][..., :3], "b": acc[..., :3] / F(spp), "c": hist["c"][..., :3]}
        filt = filtered_mask(a)
        sets = {"all": filt, "block": filt & (i == 1)}
        prev = (sc, g, a, i)
        if k in report:
            ref, _, _ = oracle.trace(sc, ob.make_request(N, N, spp=ref_spp, bounces=5), scenes.make_seeds(ref_spp, 5, base=99))
            want = ref[..., :3] / ref_spp
            res = {s: {name: float(np.sqrt(np.mean((x[m] - want[m]) ** 2))) if m.any() else float("nan") for name, m in sets.items()}
                   for s, x in planes.items()}
            res["reused"] = float((pr_a[sets["block"], 3] > 0).mean())
            res["pixels"] = {name: int(m.sum()) for name, m in sets.items()}
            out[k] = res
    return out
