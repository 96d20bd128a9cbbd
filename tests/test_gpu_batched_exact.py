"""The default (batched, overlapped) mode on a real MI355X, bit for bit against the per-sample oracle (tests/batched_oracle.py).

Bar: every ray counter equal to the oracle's, the trace accumulator's .xyz BIT-IDENTICAL to ((0 + L_0) + L_1) + ... with
L_k = ((0 + nee_0) + nee_1 + ...) + terminal from the oracle's one-sample traces, .w bit-identical to sum_k lum(L_k)^2 where moments
are on (and zero where they are off) -- whatever samples_per_batch, overlap and the kernel family are.

The cases are the shapes at which k_fold_nee and k_resolve can go wrong: bounce counts around the fold's groups of four, path counts
below / at / just over one 256-path chunk, partial last chunks, row blocks that do not start at pixel 0, short last batches, batches
larger than the sample count, one to three batches in flight, chunks without a single shadow ray, and every kernel family that writes
the visibility bytes the fold reads.
"""
import os
import sys

import numpy as np
import pytest

import batched_oracle as BO
from conftest import bits, make_hip_tracer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

pytestmark = pytest.mark.gpu

CHUNK = 256   # paths per k_fold_nee workgroup


def counters(st, B):
    return (list(st.rays_per_bounce[:B]), list(st.occl_per_bounce[:B]), st.primary_rays, st.indirect_rays, st.occlusion_rays,
            st.shaded_hits, st.shaded_misses, st.unoccluded, st.emitter_hits)


def fuzz_scene():
    """Seed 2 of the parity fuzz: an environment light, a background, three emitters, paths that run long (64 x 24)."""
    from random_scenes import random_case

    sc, c = random_case(2)
    assert sc.scene_emissive_mat_index >= 0 and sc.scene_diffuse_mat_index >= 0
    return sc, c["W"], c["H"]


def scene_of(name):
    from polaris_amd import scenes

    if name == "fuzz-env":
        return fuzz_scene()
    W, H = 70, 33   # 2 310 paths: nine chunks and a partial one
    return scenes.SCENES[name](W / H), W, H


class Case:
    """One frame: the oracle's per-sample reference (computed once, with the moments plane) and the HIP traces compared with it."""

    def __init__(self, oracle, sc, W, H, spp, B, rr=3, by=0, bh=None, base=77):
        from oracle import pybind as ob
        from polaris_amd import scenes

        self.sc, self.W, self.H, self.spp, self.B = sc, W, H, spp, B
        self.by, self.bh = by, (H - by if bh is None else bh)
        self.seeds = scenes.make_seeds(max(spp, 1), B, base=base)
        self.make_req = lambda: ob.make_request(W, H, spp=spp, bounces=B, rr=rr, block_y=by, block_h=self.bh)
        self.frames, self.stats = BO.per_sample_frames(oracle, sc, self.make_req, self.seeds, spp, B)
        self.want = BO.sum_ascending(self.frames, (H, W, 4), moments=True)
        assert not np.isnan(self.want).any()

    def check(self, **options):
        moments = options.pop("moments", 0)
        tr = make_hip_tracer(self.sc, self.W, self.H, **options)
        try:
            if moments:
                tr.set_option("moments", 1)
            req = self.make_req()
            tr.Trace(req, self.seeds)
            got, gs = tr.read_accumulator(0), tr.last_trace_stats
            assert req.accumulated_samples == self.spp
        finally:
            tr.Close()
        what = (self.sc.name, self.W, self.H, self.by, self.bh, self.spp, self.B, options, moments)
        rows = slice(self.by, self.by + self.bh)
        assert counters(gs, self.B) == counters(self.stats, self.B), what
        differing = int((bits(got[rows, :, :3]) != bits(self.want[rows, :, :3])).sum())
        assert np.array_equal(bits(got[rows, :, :3]), bits(self.want[rows, :, :3])), (what, f"{differing} accumulator words differ")
        if moments:
            assert np.array_equal(bits(got[rows, :, 3]), bits(self.want[rows, :, 3])), what
        else:
            assert not bits(got[rows, :, 3]).any(), what
        return got


@pytest.mark.parametrize("name", ["cornell", "fuzz-env"])
@pytest.mark.parametrize("B,rr", [(0, 1), (1, 2), (3, 4), (4, 5), (5, 6), (8, 9), (9, 10), (32, 33), (32, 0), (5, 3)])
def test_bounce_counts_round_the_folds_groups_of_four(built, oracle, name, B, rr):
    """0 bounces: nothing is shaded, no fold (the accumulator stays zero); 4 and 8: whole groups of four; 1, 3, 5, 9: a ragged last group;
    32: the maximum.  Russian roulette is off (rr = B + 1, what the command line makes of "disabled") so that paths run their full
    length -- asserted on the oracle's counters; (32, 0) is roulette from the first bounce, (5, 3) the headline's setting."""
    sc, W, H = scene_of(name)
    c = Case(oracle, sc, W, H, 3, B, rr=rr)
    if B == 0:
        assert c.stats.total_rays() == W * H * 3 and not c.want.any()
    else:
        assert c.stats.occlusion_rays > 0 and c.stats.unoccluded > 0 and c.want[..., :3].any()
        if rr > B:
            assert c.stats.rays_per_bounce[B - 1] > 0 and c.stats.occl_per_bounce[B - 1] > 0   # paths reach the last bounce
    c.check(samples_per_batch=2, overlap=2)
    c.check(moments=1)


SHAPES = [(1, 1, 0, 1), (255, 1, 0, 1), (256, 1, 0, 1), (257, 3, 1, 2), (70, 9, 4, 1), (97, 71, 13, 21)]


@pytest.mark.parametrize("W,H,by,bh", SHAPES)
def test_frame_shapes_round_one_chunk(built, oracle, W, H, by, bh):
    """N = 1, 255, 256 (below and at one chunk), 514 (two chunks and two paths), 70, 2 037 (a partial last chunk) paths; three of the
    blocks start at a row other than 0 (k_resolve's pixel0)."""
    from polaris_amd import scenes

    c = Case(oracle, scenes.SCENES["cubes"](W / H), W, H, 3, 5, by=by, bh=bh)
    assert c.stats.primary_rays == W * bh * 3
    c.check()
    c.check(samples_per_batch=2, overlap=2, moments=1)


BATCHES = [(1, 1, 1), (5, 1, 3), (5, 2, 2), (7, 3, 3), (6, 6, 1), (4, 9, 2)]


@pytest.mark.parametrize("W,H,by,bh", [(255, 1, 0, 1), (257, 3, 1, 2), (97, 71, 13, 21)])
def test_batch_size_and_overlap_do_not_change_a_bit(built, oracle, W, H, by, bh):
    """(spp, samples_per_batch, overlap): a short last batch (5 / 2, 7 / 3), a batch larger than the sample count (4 / 9), one to three
    batches in flight.  Every combination equals the per-sample sum of its sample count; the two of 5 spp are therefore equal to each
    other too (asserted directly as well)."""
    from polaris_amd import scenes

    sc = scenes.SCENES["cubes"](W / H)
    cases, got = {}, {}
    for i, (spp, batch, overlap) in enumerate(BATCHES):
        if spp not in cases:
            cases[spp] = Case(oracle, sc, W, H, spp, 4, by=by, bh=bh, base=5)
        got[spp, batch, overlap] = cases[spp].check(samples_per_batch=batch, overlap=overlap, moments=i % 2)
    assert np.array_equal(bits(got[5, 1, 3][..., :3]), bits(got[5, 2, 2][..., :3]))


def test_chunks_without_a_shadow_ray(built, oracle):
    """The camera looks at the horizon of the sphere scene (background + environment light) in a frame of 256 x 6: a row is one chunk.
    The top row's paths all miss -- a terminal term each, no shadow ray in any bounce: k_fold_nee's `any == 0` return -- the bottom
    row's all hit.  The precondition is asserted on the oracle (primary-hit tap and accumulator of every sample), not on HIP."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    W, H, spp, B = CHUNK, 6, 3, 4
    sc = scenes.SCENES["sphere"](1.0)
    sc.set_camera(eye=(0, 1.6, 4.5), look=(0, 1.6, 0), fov=0.75, aspect=1.0)
    c = Case(oracle, sc, W, H, spp, B, base=9)
    stride = 1 + B
    for k in range(spp):
        x, st, taps = oracle.trace(sc, ob.make_request(W, H, spp=1, bounces=B), c.seeds[k * stride:(k + 1) * stride], tap_sample=0)
        assert np.array_equal(bits(x), bits(c.frames[k]))
        hit = taps["primary_hit"].reshape(H, W) != 0
        lit = x[..., :3].sum(axis=-1) > 0
        assert not hit[0].any() and lit[0].all(), k                 # chunk 0 of sample k: all miss, every terminal non-zero
        assert hit[H - 1].all() and lit[H - 1].any(), k             # its last chunk: hits, radiance from shadow rays and terminals
        assert hit[1:H - 1].any() and not hit[1:H - 1].all(), k     # chunks in between hold both kinds of path
    assert c.stats.unoccluded > 0 and c.stats.shaded_misses >= spp * W
    for opts in ({}, {"samples_per_batch": 1, "overlap": 3}, {"samples_per_batch": 2, "overlap": 2, "moments": 1}, {"traversal": 0, "moments": 1}):
        c.check(**opts)


@pytest.mark.parametrize("name", ["cornell", "fuzz-env"])
def test_every_kernel_family_that_writes_the_visibility_bytes(built, oracle, name):
    """The batched path through k_occlusion (traversal = 0), k_trace (default) and the wave-packet shadow kernel (packet_shadow = 32),
    each with the per-wave shade kernel on and off, each with and without moments."""
    sc, W, H = scene_of(name)
    c = Case(oracle, sc, W, H, 5, 5)
    assert c.stats.unoccluded > 0 and c.stats.occlusion_rays > c.stats.unoccluded
    for family in ({"traversal": 0}, {}, {"packet_shadow": 32}):
        for shade_wave in (0, 1):
            for moments in (0, 1):
                c.check(samples_per_batch=2, overlap=2, shade_wave=shade_wave, moments=moments, **family)
