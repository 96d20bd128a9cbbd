"""The shade kernels' prefilter (option shade_prefilter, kernels.h shade_fate) on a real MI355X.

Before shade_ray the shade kernels retire the rays that only count: a ray that left a scene without a background, and a ray Russian
roulette rejects on a hit whose shading class cannot end in an emitter.  k_shade (SORT) keeps them out of the class sort, the unsorted
k_shade variants skip shade_ray for them, k_shade_wave screens a group's rays first and shades the survivors from a per-wave queue.
None of it may show:

* exact mode is BIT-IDENTICAL to the CPU oracle's accumulator,
* batched mode is BIT-IDENTICAL to the per-sample sum (tests/batched_oracle.py),
* in both every counter of test_gpu_parity.counters() plus emitter_hits equals the oracle's,

with the prefilter on (default) and off, through every shade kernel and wherever roulette starts.
Frames are 96 x 80, 6 spp, 5 bounces unless a test says otherwise (30 chunks a sample, workgroups straddling rows).
"""
import numpy as np
import pytest

from batched_oracle import per_sample_reference
from conftest import bits, make_hip_tracer
from test_gpu_parity import counters

pytestmark = pytest.mark.gpu

W, H, SPP, B = 96, 80, 6, 5
_REF = {}


def _scene(name):
    from polaris_amd import scenes

    if name == "glowing-walls":
        return glowing_walls_scene()
    return scenes.SCENES[name]()


def reference(oracle, name, rr, w=W, h=H, spp=SPP, nb=B):
    """(scene, seeds, oracle accumulator, oracle stats, per-sample sum): computed once per case and shared, never written to."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    key = (name, rr, w, h, spp, nb)
    if key not in _REF:
        sc = _scene(name)
        seeds = scenes.make_seeds(spp, nb, base=4321)
        want, ws, _ = oracle.trace(sc, ob.make_request(w, h, spp=spp, bounces=nb, rr=rr), seeds)
        per_sample, ps = per_sample_reference(oracle, sc, lambda: ob.make_request(w, h, spp=spp, bounces=nb, rr=rr), seeds, spp, nb)
        assert counters(ps, nb) == counters(ws, nb) and ps.emitter_hits == ws.emitter_hits
        for a in (want, per_sample):
            a.setflags(write=False)
        _REF[key] = (sc, seeds, want, ws, per_sample)
    return _REF[key]


def hip_trace(sc, seeds, rr, opts, w=W, h=H, spp=SPP, nb=B, repeat=1):
    from oracle import pybind as ob

    tr = make_hip_tracer(sc, w, h, **opts)
    try:
        out = []
        for _ in range(repeat):
            tr.Trace(ob.make_request(w, h, spp=spp, bounces=nb, rr=rr), seeds)
            out.append((tr.read_accumulator(0), tr.last_trace_stats))
    finally:
        tr.Close()
    return out if repeat > 1 else out[0]


def check(ref, rr, opts, exact, what, **shape):
    """One HIP trace against the bars of this file; returns its accumulator."""
    sc, seeds, want, ws, per_sample = ref
    nb = shape.get("nb", B)
    o = dict(opts)
    if exact:
        o["exact_accumulate"] = 1
    got, gs = hip_trace(sc, seeds, rr, o, **shape)
    assert counters(gs, nb) == counters(ws, nb), what
    assert gs.emitter_hits == ws.emitter_hits, what
    assert np.array_equal(bits(got[..., :3]), bits((want if exact else per_sample)[..., :3])), what
    return got


@pytest.mark.parametrize("rr", [0, 1, 3, 5])
@pytest.mark.parametrize("name", ["cornell", "sphere", "many-materials", "materials"])
def test_wherever_roulette_starts(built, oracle, name, rr):
    """Roulette from bounce 0 (camera rays, in the FIRST kernel), 1, 3 (the default) and 5 (nowhere): an open box, an environment light
    (misses are shaded, nothing escapes), more reach sets than classes (class 15 is shared) and textured operators."""
    ref = reference(oracle, name, rr)
    for exact in (True, False):
        check(ref, rr, {}, exact, (name, rr, exact))


OPTION_SETS = [{"shade_sort": 32}, {"shade_wave": 0}, {"shade_wave_from": 0}, {"shade_wave_from": 1}, {"stage_lds": 0},
               {"samples_per_batch": 1}, {"samples_per_batch": 4}, {"overlap": 3}]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", ["cornell", "many-materials"])
def test_every_shade_path(built, oracle, name, opts):
    """Unsorted k_shade, k_shade without k_shade_wave, k_shade_wave from the first bounce it can take, tables in global memory, batch sizes
    and batches in flight: each with the prefilter off and on, equal to each other and to the oracle.  (samples_per_batch and overlap
    shape batched traces only.)"""
    rr = 3
    ref = reference(oracle, name, rr)
    batched_only = "samples_per_batch" in opts or "overlap" in opts
    for exact in ((False,) if batched_only else (True, False)):
        default = check(ref, rr, {}, exact, (name, "defaults", exact))
        off = check(ref, rr, dict(opts, shade_prefilter=0), exact, (name, opts, exact, "off"))
        on = check(ref, rr, dict(opts, shade_prefilter=1), exact, (name, opts, exact, "on"))
        assert np.array_equal(bits(off), bits(on)) and np.array_equal(bits(on), bits(default)), (name, opts, exact)


def glowing_walls_scene():
    """A closed room whose walls are mix(emissive, diffuse): every wall hit belongs to a class that CAN end in an emitter, so a ray that
    roulette rejects there may still add radiance and must not be retired.  A plain diffuse block stands in it (a class that cannot)."""
    from polaris_amd import scenes as S

    mt = S.MaterialTable()
    glow = mt.mix(mt.emissive((0.9, 0.7, 0.4), 1.0), mt.diffuse((0.6, 0.6, 0.6)), 0.35)
    grey = mt.diffuse((0.5, 0.5, 0.5))
    parts = [
        S.quad((1, 0, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1), glow),   # floor
        S.quad((1, 1, 0), (1, 1, 1), (0, 1, 1), (0, 1, 0), glow),   # ceiling
        S.quad((1, 0, 1), (0, 0, 1), (0, 1, 1), (1, 1, 1), glow),   # back
        S.quad((0, 0, 1), (0, 0, 0), (0, 1, 0), (0, 1, 1), glow),   # right
        S.quad((1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0), glow),   # left
        S.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), glow),   # front (behind the camera's near side: faces inwards)
        S.box((0.3, 0.0, 0.4), (0.7, 0.5, 0.8), grey, rot_y=0.3),
    ]
    sc = S.compile_scene([S.merge(parts)], [(0, np.eye(4))], mt, name="glowing-walls")
    sc.set_camera(eye=(0.5, 0.5, 0.05), look=(0.5, 0.4, 1.0), fov=0.9, aspect=W / H)
    return sc


def test_an_emitter_behind_a_mix(built, oracle):
    """Rejected rays that land on a class that can emit.  Not vacuous: the oracle counts emitter hits at bounces >= min_rr (all its
    emitter hits less those of the camera rays, which a one-bounce trace with the same camera and first shade seeds counts)."""
    from oracle import pybind as ob

    rr = 1
    ref = reference(oracle, "glowing-walls", rr)
    sc, seeds, _, ws, _ = ref
    first = np.ascontiguousarray(np.asarray(seeds, np.uint32).reshape(SPP, 1 + B)[:, :2])  # per sample: camera seed, shade seed of bounce 0
    _, s0, _ = oracle.trace(sc, ob.make_request(W, H, spp=SPP, bounces=1, rr=rr), first.reshape(-1))
    assert s0.rays_per_bounce[0] == ws.rays_per_bounce[0]
    assert ws.emitter_hits - s0.emitter_hits > 0, "no emitter hit at a roulette bounce: the case checks nothing"
    assert ws.rays_per_bounce[1] - ws.rays_per_bounce[2] > ws.emitter_hits, "no ray was rejected"
    for opts in ({}, {"shade_wave_from": 1}, {"shade_wave": 0}, {"shade_sort": 32, "shade_wave": 0}):
        for exact in (True, False):
            check(ref, rr, opts, exact, (opts, exact))


@pytest.mark.parametrize("shape", [(8, 8, 6, 5), (300, 1, 6, 5), (96, 80, 6, 12)], ids=lambda s: "x".join(map(str, s)))
def test_queue_edges_of_the_wave_kernel(built, oracle, shape):
    """k_shade_wave from bounce 1 with roulette from bounce 1: one partly filled chunk; two chunks of one group; 180 chunks in 23 groups,
    the last of 4 chunks, groups straddling samples.  The big frame runs 12 bounces so that its last bounces are nearly empty."""
    w, h, spp, nb = shape
    rr = 1
    ref = reference(oracle, "cornell", rr, w, h, spp, nb)
    ws = ref[3]
    if (w, h) == (96, 80):
        # From the counters, by counting: a survivor is a ray of the bounce, and every ray of the next bounce has a survivor as its parent.
        chunks = spp * ((w * h + 255) // 256)
        groups = (chunks + 7) // 8
        assert (chunks, groups, chunks % 8) == (180, 23, 4)
        rays = list(ws.rays_per_bounce[:nb])
        assert any(rays[b + 1] > 64 * groups for b in range(1, nb - 1)), "no group is sure to queue more than one pass of survivors"
        assert any(0 < rays[b] < groups for b in range(1, nb)), "no bounce is sure to leave a group without a survivor"
    for opts in ({"shade_wave_from": 1}, {"shade_wave_from": 1, "shade_prefilter": 0}):
        for exact in (True, False):
            check(ref, rr, opts, exact, (shape, opts, exact), w=w, h=h, spp=spp, nb=nb)


def test_determinism_with_four_batches_in_flight(built, oracle):
    """The same Trace five times on one handle, four pipelines: equal bits every time (and the oracle's)."""
    rr = 3
    ref = reference(oracle, "cornell", rr)
    sc, seeds, _, ws, per_sample = ref
    runs = hip_trace(sc, seeds, rr, {"overlap": 4, "samples_per_batch": 1}, repeat=5)
    for got, gs in runs:
        assert counters(gs, B) == counters(ws, B) and gs.emitter_hits == ws.emitter_hits
        assert np.array_equal(bits(got), bits(runs[0][0]))
    assert np.array_equal(bits(runs[0][0][..., :3]), bits(per_sample[..., :3]))
