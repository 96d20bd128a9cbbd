"""Editing materials in place on the MI355X (polaris_hip_update_materials, polaris_hip_update_texture).

Set-up: tracer A uploads `base` and applies the case's calls; tracer B uploads `substituted` = scenes.with_materials(base, ...), the
scene the update is defined to equal; the CPU oracle traces substituted's arrays.  Bars: the device's triangle records and the shading
record (tri_bits, emit_classes, background node, slots) of A and B are byte-equal, the pair and instance records stay those of the
tracer before the update; frames, counters, shade counts, kernel symbols, probes and taps of A, of B and of the oracle are bit-equal
whatever kernels run, with the shade prefilter on and off; the temporal history is dropped; the update allocates nothing in the
scene's pool; a refused call leaves the next frame bit-equal to the frame before it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import material_update_cases as cases
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from polaris_amd import scenes
from test_gpu_denoise import sync, trace
from test_gpu_instance_update import B, H, SPP, W, counters, probe_rays

pytestmark = pytest.mark.gpu

E_NO_SCENE_DATA, E_BAD_ARGUMENT, E_BAD_SCENE = 1, 2, 5
RR_LIVE = ("new-emitter", "light-off")     # traced with min_bounces_for_rr = 1: Russian roulette decides on every bounce after the first


def rr_of(name):
    return 1 if name in RR_LIVE else 3


def updated(name, **options):
    base, _, args = cases.case(name)
    tr = make_hip_tracer(base, W, H, **options)
    cases.apply(tr, args)
    return tr


def frame(tr, rr=3, base=21):
    """(trace accumulator, counters) of one frame."""
    from oracle import pybind as ob

    tr.Trace(ob.make_request(W, H, spp=SPP, bounces=B, rr=rr), scenes.make_seeds(SPP, B, base=base))
    return tr.read_accumulator(0), counters(tr.last_trace_stats)


def same_frame(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1]


def close(*tracers):
    for tr in tracers:
        tr.Close()


# ---- 1. the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [0, -1])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_records_equal_a_full_upload_of_the_substituted_scene(built, name, max_leaf):
    base, sub, args = cases.case(name)
    a, b = make_hip_tracer(base, W, H, max_leaf_tris=max_leaf), make_hip_tracer(sub, W, H, max_leaf_tris=max_leaf)
    try:
        tris0, shading0, rec0, counts0 = a.read_triangle_records(), a.read_shading_record(), a.read_scene_records(), a.scene_counts()
        a.set_option("time_kernels", 1)
        cases.apply(a, args)
        tris, shading = a.read_triangle_records(), a.read_shading_record()
        assert tris.tobytes() == b.read_triangle_records().tobytes(), "triangle records"
        assert shading == b.read_shading_record() and shading[0] == 24 and shading[3] == len(tris)
        rec = a.read_scene_records()
        assert rec[0].tobytes() == rec0[0].tobytes() and rec[1].tobytes() == rec0[1].tobytes(), "pair and instance records"
        assert a.scene_counts() == counts0 == b.scene_counts(), "the update allocates nothing in the scene's pool"
        assert (shading[1] != shading0[1]) == (name in cases.MASK_CHANGES)
        if name == "recolour":
            assert tris.tobytes() == tris0.tobytes()
        if name in ("retype", "reassign", "textured", "not-tiny", "new-emitter"):
            assert tris.tobytes() != tris0.tobytes()
        if name == "background":
            assert shading[2] == -1 and shading0[2] >= 0
        assert (len(tris) > 2046) == (name == "not-tiny")
        assert a.kernel_symbol("retag") == "pol::k_retag" and a.kernel_ms("retag")[1] == 1
    finally:
        close(a, b)


# ---- 2. results ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_results(name):
    """What the CPU oracle makes of the substituted scene, once per case."""
    from oracle import pybind as ob

    _, sub, _ = cases.case(name)
    oracle = ob.Oracle("oracle")
    seeds = scenes.make_seeds(SPP, B, base=21)
    want, ws, wt = oracle.trace(sub, ob.make_request(W, H, spp=SPP, bounces=B, rr=rr_of(name)), seeds, tap_sample=0)
    return seeds, want, ws, wt


def variants(name):
    out = [{}, {"traversal": 0}, {"node_mode": 0}, {"node_mode": 1}, {"packet_primary": 1}]
    return out if name == "not-tiny" else out + [{"node_mode": 2}]


@pytest.mark.parametrize("prefilter", [1, 0])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_results_equal_a_full_upload_and_the_oracle(built, oracle, name, prefilter):
    from oracle import pybind as ob

    _, sub, _ = cases.case(name)
    seeds, want, ws, wt = oracle_results(name)
    rr = rr_of(name)
    changed = False
    for opts in variants(name):
        opts = dict(opts, shade_prefilter=prefilter)
        a, b = updated(name, **opts), make_hip_tracer(sub, W, H, **opts)
        try:
            for tr in (a, b):
                tr.set_option("time_kernels", 1)
            fa, fb = frame(a, rr), frame(b, rr)                 # batched, all counters
            assert same_frame(fa, fb), opts
            assert fa[1][:2] == (list(ws.rays_per_bounce[:B]), list(ws.occl_per_bounce[:B])), opts
            for k in ("intersect", "occlusion") + a.SHADE_TIMERS:
                assert a.kernel_symbol(k) == b.kernel_symbol(k), (k, opts)
            assert a.kernel_symbol("intersect") + a.kernel_symbol("intersect_packet") != "" and any(a.kernel_symbol(k) for k in a.SHADE_TIMERS)
            assert a.shade_counts(B) == b.shade_counts(B), opts
            for tr in (a, b):
                tr.set_option("exact_accumulate", 1)
            ea, eb = frame(a, rr), frame(b, rr)
            assert same_frame(ea, eb), opts
            assert np.array_equal(bits(ea[0][..., :3]), bits(want[..., :3])), opts
            req = ob.make_request(W, H, spp=SPP, bounces=B, rr=rr)
            ta, tb = a.tap_primary(req, int(seeds[0])), b.tap_primary(req, int(seeds[0]))
            for k in ta:
                assert np.array_equal(bits(ta[k]), bits(tb[k])), (k, opts)
            for k in ("primary_hit", "primary_wuvt", "primary_tri"):
                assert np.array_equal(bits(ta[k]), bits(np.asarray(wt[k]).reshape(ta[k].shape))), (k, opts)
            if not changed:                                     # the edit shows: the base's own frame is another one
                c = make_hip_tracer(cases.case(name)[0], W, H, **opts)
                try:
                    c.set_option("exact_accumulate", 1)
                    assert not np.array_equal(bits(frame(c, rr)[0]), bits(ea[0])), "the case changes no pixel"
                finally:
                    c.Close()
                changed = True
        finally:
            close(a, b)


def test_roulette_is_live_on_the_bounces_traced(built):
    """Cases 3 and 4 are traced with min_bounces_for_rr = 1 and three bounces: rays do end in roulette there (fewer rays on a later
    bounce than without it), so the prefilter's promise -- a clear bit of emit_classes -- is exercised by the mask the update wrote."""
    for name in RR_LIVE:
        a = updated(name)
        try:
            with_rr, without = frame(a, 1)[1], frame(a, B + 1)[1]
            assert B >= 3 and sum(with_rr[0]) < sum(without[0]), name
        finally:
            a.Close()


# ---- 3. probes -----------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("name", ["textured", "retype", "light-off"])
def test_probes_equal_a_full_upload_and_the_oracle(built, oracle, name):
    """polaris_hip_probe of every kind, on the input grids of tests/test_gpu_probes.py (fewer random rows; the oracle, a call per
    row, judges the first ORACLE_ROWS of each, which hold every degenerate row): every BxDF leaf, every texture (after
    update_texture), every emissive, the material walk from every node."""
    _, sc, _ = cases.case(name)
    rng = np.random.default_rng(21)
    n, ORACLE_ROWS = 200, 24
    a, b = updated(name), make_hip_tracer(sc, W, H)
    try:
        for stage_lds in (1, 0):
            for tr in (a, b):
                tr.set_option("stage_lds", stage_lds)
            for leaf in [i for i, m in enumerate(sc.material_nodes) if 4 <= int(m["type"]) < T.OP_MIX]:
                nrm, wi, wo = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
                uv = rng.uniform(-2, 3, size=(n, 2)).astype(np.float32)
                xi = rng.random((n, 2)).astype(np.float32)
                wi[0] = nrm[0]; wi[1] = -nrm[1]
                wi[2:6] = unit(np.cross(nrm[2:6], rng.normal(size=(4, 3))))
                wo[6] = (2.0 * np.dot(wi[6], nrm[6]) * nrm[6] - wi[6]).astype(np.float32)
                xi[7] = (0.0, 0.0); xi[8] = (np.float32(1.0) - np.float32(2.0 ** -24), 0.5); xi[9] = (0.5, 0.0)
                uv[10] = (0.0, 0.0); uv[11] = (1.0, 1.0); uv[12] = (-0.25, 1.75)
                rows = np.concatenate([nrm, uv, wi, xi, wo], axis=1)
                got = a.probe(a.PROBE_BXDF, leaf, rows)
                assert same_bits(got, b.probe(b.PROBE_BXDF, leaf, rows)), (stage_lds, leaf)
                for r in range(ORACLE_ROWS):
                    assert same_bits(got[r], oracle.bxdf_probe(sc.material_nodes[leaf:leaf + 1], sc.texture_meta, sc.texture_data, nrm[r], uv[r], wi[r], xi[r], wo[r])), (stage_lds, leaf, r)
            edge = [(0.0, 0.0), (1.0, 1.0), (0.999999, 0.5), (-0.25, 1.75), (3.0, -2.0), (0.5, 0.0), (0.0, 0.999999), (0.9999999, 0.9999999),
                    (-1e-7, -1e-7), (1e-8, 123.456), (-0.0, 0.5)]
            for t in range(len(sc.texture_meta)):
                w, h = int(sc.texture_meta[t]["width"]), int(sc.texture_meta[t]["height"])
                grid = [((x + fx) / w, (y + fy) / h) for x in (0, w - 2, w - 1) for y in (0, h - 2, h - 1) for fx, fy in ((0.0, 0.0), (0.5, 0.5), (0.99, 0.01))]
                uvs = np.array(edge + grid + [tuple(rng.uniform(-2, 3, size=2)) for _ in range(n)], dtype=np.float32)
                got = a.probe(a.PROBE_TEXTURE, t, uvs)
                assert same_bits(got, b.probe(b.PROBE_TEXTURE, t, uvs)), (stage_lds, t)
                for r in range(len(edge) + len(grid)):
                    assert same_bits(got[r], oracle.tex_probe(sc.texture_meta, sc.texture_data, t, uvs[r])), (stage_lds, t, r)
            for e in range(len(sc.emissives)):
                p = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
                nrm, d = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
                xi = rng.random((n, 2)).astype(np.float32)
                xi[0] = (0.0, 0.0); xi[1] = (np.float32(1.0) - np.float32(2.0 ** -24), np.float32(1.0) - np.float32(2.0 ** -24))
                rows = np.concatenate([p, nrm, xi, d], axis=1)
                got = a.probe(a.PROBE_EMISSIVE, e, rows)
                assert same_bits(got, b.probe(b.PROBE_EMISSIVE, e, rows)), (stage_lds, e)
                for r in range(ORACLE_ROWS):
                    assert same_bits(got[r], oracle.emissive_probe(sc, e, p[r], nrm[r], xi[r], d[r])), (stage_lds, e, r)
            for root in range(len(sc.material_nodes)):
                nrm = unit(rng.normal(size=(n, 3)))
                uv = rng.uniform(-2, 3, size=(n, 2)).astype(np.float32)
                st = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
                flags = rng.choice([0, 0, 1, 2, 4], size=n).astype(np.uint32)
                rows = np.concatenate([nrm, uv, st.view(np.float32), flags.view(np.float32)[:, None]], axis=1)
                got = a.probe(a.PROBE_MATERIAL, root, rows)
                assert same_bits(got, b.probe(b.PROBE_MATERIAL, root, rows)), (stage_lds, root)
                for r in range(ORACLE_ROWS):
                    assert same_bits(got[r], oracle.material_probe(sc, root, nrm[r], uv[r], st[r], int(flags[r]))), (stage_lds, root, r)
        rays = probe_rays(sc, n=4000)
        for any_hit in (False, True):
            ha, hb = a.probe_intersect(rays, any_hit=any_hit), b.probe_intersect(rays, any_hit=any_hit)
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(ha, hb)), any_hit
    finally:
        close(a, b)


# ---- 4. G-buffer and history ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["retype", "textured"])
def test_gbuffer_after_the_update_equals_a_full_upload(built, name):
    base, sub, args = cases.case(name)
    a, b = make_hip_tracer(base, W, H), make_hip_tracer(sub, W, H)
    try:
        stale = a.read_aov(T.AOV_ALBEDO)                        # the G-buffer of the base scene: the update must invalidate it
        cases.apply(a, args)
        for aov in (T.AOV_GUIDE, T.AOV_ALBEDO):
            assert np.array_equal(bits(a.read_aov(aov)), bits(b.read_aov(aov))), aov
        assert not np.array_equal(bits(a.read_aov(T.AOV_ALBEDO)), bits(stale))
    finally:
        close(a, b)


@pytest.mark.parametrize("texture_only", [False, True])
@pytest.mark.parametrize("object_motion", [True, False])
def test_history_is_dropped(built, object_motion, texture_only):
    name = "textured"
    base, sub, args = cases.case(name)
    if texture_only:
        args = dict(args, nodes=base.material_nodes, material_index=None)
        sub = scenes.with_materials(base, textures=args["textures"])

    def run(tr, with_update):
        try:
            tr.set_denoise(**T.DENOISE_DEFAULTS)
            tr.set_temporal(**T.TEMPORAL_DEFAULTS)
            if with_update:
                trace(tr, W, H, 4, bounces=B)
                sync(tr, W, H, 4)
                if texture_only:
                    for index, texels in args["textures"].items():
                        tr.update_texture(index, texels)
                else:
                    cases.apply(tr, args)
            trace(tr, W, H, 1, base=9, bounces=B)
            sync(tr, W, H, 1)
            return tr.read_aov(T.AOV_PRIOR), tr.read_framebuffer()
        finally:
            tr.Close()

    prior, fb = run(make_hip_tracer(base, W, H, object_motion=int(object_motion)), True)
    _, want = run(make_hip_tracer(sub, W, H, object_motion=int(object_motion)), False)
    assert not (prior[..., 3] != 0).any()                       # no history: m = 0 everywhere
    assert np.array_equal(fb, want)


# ---- 5. sequences --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["new-emitter", "background", "class-15", "not-tiny"])
def test_two_updates_equal_one_and_an_update_back_restores_the_upload(built, name):
    base, sub, args = cases.case(name)
    _, _, other = cases.case("retype" if name == "new-emitter" else name)
    rr = rr_of(name)
    a, b = make_hip_tracer(base, W, H), make_hip_tracer(base, W, H)
    try:
        tris0, shading0, f0 = a.read_triangle_records(), a.read_shading_record(), frame(a, rr)
        if name == "new-emitter":
            cases.apply(a, other)                               # another edit first ...
        else:
            cases.apply(a, args)
        cases.apply(a, args)                                    # ... then the case's: two updates
        cases.apply(b, args)                                    # one
        assert a.read_triangle_records().tobytes() == b.read_triangle_records().tobytes() and a.read_shading_record() == b.read_shading_record()
        fa = frame(a, rr)
        assert same_frame(fa, frame(b, rr)) and not np.array_equal(bits(fa[0]), bits(f0[0]))
        back = dict(nodes=base.material_nodes, material_index=base.material_index, scene_diffuse=int(base.scene_diffuse_mat_index),
                    emissive_mat_nodes=base.emissives["mat_node_index"].copy(), textures=None)
        cases.apply(a, back)
        assert a.read_triangle_records().tobytes() == tris0.tobytes() and a.read_shading_record() == shading0
        assert same_frame(frame(a, rr), f0)
    finally:
        close(a, b)


def relit(base):
    """An edit that moves every emissive entry of the first light's node to ANOTHER node: a diffuse leaf's slot becomes a copy of the
    light's leaf with its own radiance (the entry's node is what light sampling reads), and emissive_mat_nodes points there."""
    n = base.material_nodes.copy()
    old = int(base.emissives["mat_node_index"][0])
    spare = int(np.nonzero((n["type"] == T.BXDF_DIFFUSE) & (np.arange(len(n)) != base.scene_diffuse_mat_index))[0][-1])
    n[spare] = n[old]
    n["k"][spare][:3] = (3.0, 9.0, 14.0)
    nodes = np.where(base.emissives["mat_node_index"] == old, spare, base.emissives["mat_node_index"]).astype(np.uint32)
    return dict(nodes=n, material_index=None, scene_diffuse=int(base.scene_diffuse_mat_index), emissive_mat_nodes=nodes, textures=None)


@pytest.mark.parametrize("materials_first", [True, False])
@pytest.mark.parametrize("other", ["instances", "vertices"])
def test_material_updates_compose_with_the_other_two_in_either_order(built, other, materials_first):
    import vertex_update_cases as vu

    base, moved, _ = vu.case("moving-and-deformed")             # vertices and matrices change
    if other == "instances":
        moved = scenes.refit_instances(base, scenes.moving_instances(1))
    args = relit(base)
    both = scenes.with_materials(moved, nodes=args["nodes"], emissive_mat_nodes=args["emissive_mat_nodes"])
    a, b = make_hip_tracer(base, W, H, vertex_update=1), make_hip_tracer(both, W, H)

    def geometry(tr, ems):
        if other == "instances":
            inv, boxes, _ = scenes.instance_update_args(moved)
            tr.update_instances(inv, boxes, ems)
        else:
            vertices, boxes, normals, inv, _ = scenes.vertex_update_args(moved)
            tr.update_vertices(vertices, boxes, normals, inv, ems)

    try:
        if materials_first:
            cases.apply(a, args)
            geometry(a, both.emissives)                         # the NEW list is accepted: the handle's host copy followed the edit
        else:
            geometry(a, moved.emissives)
            cases.apply(a, args)
        ra, rb = a.read_scene_records(), b.read_scene_records()
        assert ra[1].tobytes() == rb[1].tobytes() and a.read_shading_record() == b.read_shading_record()
        assert same_frame(frame(a), frame(b))
        for tr in (a, b):
            tr.set_option("exact_accumulate", 1)
        assert same_frame(frame(a), frame(b))
    finally:
        close(a, b)


def test_an_instance_update_without_a_list_keeps_the_updated_material_nodes(built):
    """The host-copy trap: with instance_update on the handle keeps the emissive list and re-sends WHOLE entries when an update passes
    no list.  After update_materials moved the entries' nodes, an update_instances without a list must leave them moved, and one that
    passes the old list must be refused as differing."""
    base = scenes.moving_instances(0)
    moved = scenes.refit_instances(base, scenes.moving_instances(1))
    args = relit(base)
    both = scenes.with_materials(moved, nodes=args["nodes"], emissive_mat_nodes=args["emissive_mat_nodes"])
    a, b = make_hip_tracer(base, W, H, instance_update=1), make_hip_tracer(both, W, H)
    try:
        cases.apply(a, args)
        inv, boxes, _ = scenes.instance_update_args(moved)
        u, keep = T.instance_update(inv, boxes, moved.emissives)            # the list with the nodes of BEFORE the edit
        assert a._lib.polaris_hip_update_instances(a._h, C.byref(u)) == E_BAD_ARGUMENT
        assert b"differs from the uploaded one" in a._lib.polaris_hip_last_error(a._h)
        a.update_instances(inv, boxes, None)
        fa, fb = frame(a), frame(b)
        assert same_frame(fa, fb)
        c = make_hip_tracer(moved, W, H)
        try:
            assert not np.array_equal(bits(frame(c)[0]), bits(fa[0])), "the relit light looks like the old one"
        finally:
            c.Close()
    finally:
        close(a, b)


# ---- 6. untouched when unused, refusals ----------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_next_frame_as_the_one_before(built):
    from polaris_amd.tracer import ErrNoSceneData, HipTracer
    from test_material_update_cpu import _refusals, refusal_struct

    base, _, args = cases.case("textured")
    tr = make_hip_tracer(base, W, H)
    try:
        f0, tris0, shading0, counts0 = frame(tr), tr.read_triangle_records(), tr.read_shading_record(), tr.scene_counts()
        for what, status, text, bad, fields in _refusals():
            u, keep = refusal_struct(bad, fields)
            rc = tr._lib.polaris_hip_update_materials(tr._h, C.byref(u))
            assert rc == status, (what, rc)
            assert text.encode() in tr._lib.polaris_hip_last_error(tr._h), what
            assert tr.read_triangle_records().tobytes() == tris0.tobytes() and tr.read_shading_record() == shading0, what
            assert same_frame(frame(tr), f0), what
        assert tr._lib.polaris_hip_update_materials(tr._h, None) == E_BAD_ARGUMENT
        texels = np.ascontiguousarray(args["textures"][2])
        for index, n_bytes in ((len(base.texture_meta), texels.nbytes), (2, texels.nbytes - 4), (2, texels.nbytes + 4)):
            assert tr._lib.polaris_hip_update_texture(tr._h, index, texels.ctypes.data, n_bytes) == E_BAD_ARGUMENT
            assert same_frame(frame(tr), f0), (index, n_bytes)
        assert tr._lib.polaris_hip_update_texture(tr._h, 2, None, texels.nbytes) == E_BAD_ARGUMENT
        assert tr.scene_counts() == counts0
    finally:
        tr.Close()
    early = HipTracer("early", 0)
    early.Init()
    try:
        with pytest.raises(ErrNoSceneData):
            cases.apply(early, args)
        with pytest.raises(ErrNoSceneData):
            early.update_texture(2, args["textures"][2])
    finally:
        early.Close()


# ---- 7. the host layer ---------------------------------------------------------------------------------------------------------
def test_renderer_forwards_the_update_to_every_tracer(built):
    from polaris_amd import host_api

    host_api.load()
    base, sub, args = cases.case("textured")
    spp = 2

    def render(r):
        for t in range(2):
            r.push_seeds(t, scenes.make_seeds(spp, B, base=31 + t))
        r.render()
        return r.read()

    a = host_api.Renderer(base, [0, 0], width=W, height=H, spp=spp, bounces=B, seed=4)
    b = host_api.Renderer(sub, [0, 0], width=W, height=H, spp=spp, bounces=B, seed=4)
    try:
        f0 = render(a)
        with pytest.raises(RuntimeError, match="material nodes, the uploaded scene has"):
            a.update_materials(args["nodes"][:-1], None, args["scene_diffuse"])
        a.update_materials(args["nodes"], args["material_index"], args["scene_diffuse"], args["emissive_mat_nodes"])
        for index, texels in args["textures"].items():
            a.update_texture(index, texels)
        fa, fb = render(a), render(b)
        assert np.array_equal(bits(fa[1]), bits(fb[1])) and np.array_equal(fa[0], fb[0])
        assert not np.array_equal(bits(fa[1]), bits(f0[1]))
    finally:
        a.close()
        b.close()
