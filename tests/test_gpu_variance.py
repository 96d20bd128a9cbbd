"""Variance guidance on the MI355X (include/polaris_hip.h: option "moments", polaris_hip_set_variance, POLARIS_AOV_VARIANCE / _PRIOR2,
polaris_hip_variance_planes).

Bars: the moments leave .rgb and every counter bit for bit as they are and put exactly sum_k lum(x_k)^2 into .w, through the resolve
and every merge path; exact mode refuses them; k_variance and the guided filter are bit-equal to the CPU restatement
(polaris_host_variance / _denoise_variance / _reproject_moments) on caller planes and on the real path, with and without temporal
reuse; variance on with denoise off, and sigma_variance = 0, leave the frame-buffer bytes as they are without the feature; on the
device the guided filter meets the quality bars of DESIGN.md section 10c."""
import dataclasses

import numpy as np
import pytest

import gbuffer_oracle as G
import variance_oracle as VO
from batched_oracle import per_sample_reference
from conftest import bits, make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

F = np.float32
VA = T.VARIANCE_DEFAULTS
DN = T.DENOISE_DEFAULTS


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def lum2(x):
    lx = VO.lum(x[..., :3])
    return lx * lx


def seeds_of_sample(k, spp, bounces=5, base=7):
    from polaris_amd import scenes

    return scenes.make_seeds(spp, bounces, base=base)[k * (1 + bounces):(k + 1) * (1 + bounces)]


def moved(sc, dx, dy=0.0):
    return dataclasses.replace(sc, eye=(np.asarray(sc.eye, F) + np.array([dx, dy, 0], F)).astype(F))


# ---- 1-3. the moments on the trace path -----------------------------------------------------------------------------------------
def test_moments_leave_rgb_and_counters_and_w_is_zero_without(built):
    from polaris_amd import scenes

    W, H = 80, 64
    sc = scenes.SCENES["cornell"](W / H)
    out = {}
    for on in (False, True):
        tr = make_hip_tracer(sc, W, H, samples_per_batch=4)
        try:
            if on:
                tr.set_option("moments", 1)
            st = trace(tr, W, H, 16, base=3)
            out[on] = (tr.read_accumulator(0), tr.read_accumulator(1), bytes(st))
        finally:
            tr.Close()
    off, on = out[False], out[True]
    for k in (0, 1):
        assert np.array_equal(bits(off[k][..., :3]), bits(on[k][..., :3]))
        assert np.all(bits(off[k][..., 3]) == 0)
    assert off[2][:-8] == on[2][:-8]                                      # every counter (device_ms, the last field, is a time)
    assert (on[0][..., 3] > 0).mean() > 0.5 and np.array_equal(bits(on[0][..., 3]), bits(on[1][..., 3]))


def test_one_sample_is_the_square_of_its_luminance(built):
    from polaris_amd import scenes

    W, H = 80, 64
    sc = scenes.SCENES["cornell"](W / H)
    tr = make_hip_tracer(sc, W, H)
    try:
        tr.set_option("moments", 1)
        trace(tr, W, H, 1, base=11)
        acc = tr.read_accumulator(0)
    finally:
        tr.Close()
    assert np.array_equal(bits(acc[..., 3]), bits(lum2(acc)))


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_per_sample_sum_in_ascending_order(built, oracle, batch):
    """Every sample's per-path radiance is added to the accumulator one by one in ascending k, whatever the batch size,
    so the sum of L^2 of an 8 spp trace equals the float32 sum of lum(x_k)^2 of eight one-sample traces fed sample k's seeds -- HIP's
    own one-sample traces, and the CPU oracle's (tests/batched_oracle.py), which no HIP kernel has touched."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    W, H, spp = 64, 48, 8
    sc = scenes.SCENES["cornell"](W / H)
    tr = make_hip_tracer(sc, W, H, samples_per_batch=batch)
    try:
        tr.set_option("moments", 1)
        trace(tr, W, H, spp, base=7)
        got = tr.read_accumulator(1)
        xs = []
        for k in range(spp):
            tr.Trace(ob.make_request(W, H, spp=1, bounces=5), seeds_of_sample(k, spp))
            xs.append(tr.read_accumulator(0))
    finally:
        tr.Close()
    want = VO.moments_of_samples(xs)
    assert np.array_equal(bits(got[..., :3]), bits(want[..., :3]))
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3]))
    per_sample, _ = per_sample_reference(oracle, sc, lambda: ob.make_request(W, H, spp=spp, bounces=5), scenes.make_seeds(spp, 5, base=7), spp, 5, moments=True)
    assert np.array_equal(bits(got[..., :3]), bits(per_sample[..., :3]))
    assert np.array_equal(bits(got[..., 3]), bits(per_sample[..., 3]))


# ---- 4. merges --------------------------------------------------------------------------------------------------------------------
def test_w_survives_local_and_slot_merges(built):
    from oracle import pybind as ob
    from polaris_amd import scenes

    W, H, spp = 64, 48, 4
    sc = scenes.SCENES["cornell"](W / H)
    src = make_hip_tracer(sc, W, H)
    dsts = [make_hip_tracer(sc, W, H) for _ in range(2)]
    try:
        src.set_option("moments", 1)
        for d in dsts:
            d.set_option("moments", 1)
        src.ipc_export(2)
        req = ob.make_request(W, H, spp=spp, bounces=5)
        src.Trace(req, scenes.make_seeds(spp, 5, base=5))
        block = src.read_accumulator(0)
        slot = src.trace_slot()
        dsts[0].MergeOutput(src, req)
        dsts[1].merge_slot(src, slot, req)
        got = [d.read_accumulator(1) for d in dsts]
        counts = [d.merge_counts() for d in dsts]
    finally:
        src.Close()
        for d in dsts:
            d.Close()
    assert (block[..., 3] > 0).mean() > 0.5
    for g in got:
        assert np.array_equal(bits(g), bits(block))
    assert counts[0]["local"] == 1 and counts[1]["local"] == 1


# The device-strip merge needs device memory of the caller's: torch provides it, and torch must create its GPU context before
# libpolaris_hip.so is loaded, so this runs in a fresh process.
STRIP_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import torch
torch.zeros(1, device="cuda:0")
from conftest import bits, make_hip_tracer
from oracle import pybind as ob
from polaris_amd import scenes
W, H, spp = 64, 48, 4
sc = scenes.SCENES["cornell"](W / H)
src, dst = make_hip_tracer(sc, W, H), make_hip_tracer(sc, W, H)
try:
    src.set_option("moments", 1)
    dst.set_option("moments", 1)
    req = ob.make_request(W, H, spp=spp, bounces=5)
    src.Trace(req, scenes.make_seeds(spp, 5, base=5))
    block = src.read_accumulator(0)
    strip = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    src.export_block(req, strip.data_ptr())
    dst.merge_device(strip.data_ptr(), req)
    got, counts = dst.read_accumulator(1), dst.merge_counts()
finally:
    src.Close()
    dst.Close()
ok = (block[..., 3] > 0).mean() > 0.5 and np.array_equal(bits(got), bits(block)) and counts["device-strip"] == 1
print("device-strip merge carries .w:", ok)
sys.exit(0 if ok else 1)
"""


def test_w_survives_the_device_strip_merge(built):
    import subprocess
    import sys

    from conftest import ROOT

    p = subprocess.run([sys.executable, "-c", STRIP_CHILD, ROOT], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]


def test_three_block_frame_equals_each_blocks_trace_accumulator(built):
    """The frame loop by hand: three tracers trace a row block each with seeds of their own, the primary merges all three; with
    moments on, the primary's frame accumulator equals, row block by row block, that block's trace accumulator -- .w included, bit
    for bit (each row is merged once onto a cleared frame)."""
    from oracle import pybind as ob
    from polaris_amd import scenes

    W, H, spp = 96, 90, 8
    sc = scenes.SCENES["cornell"](W / H)
    trs = [make_hip_tracer(sc, W, H) for _ in range(3)]
    primary = trs[1]
    try:
        for t in trs:
            t.set_option("moments", 1)
        reqs = [ob.make_request(W, H, spp=spp, bounces=5, block_y=30 * k, block_h=30) for k in range(3)]
        order = [1, 0, 2]                                                    # the primary first: its Trace clears its frame
        blocks = {}
        for k in order:
            trs[k].Trace(reqs[k], scenes.make_seeds(spp, 5, base=40 + k))
            blocks[k] = trs[k].read_accumulator(0)[30 * k:30 * (k + 1)]
        for k in order:
            primary.MergeOutput(trs[k], reqs[k])
        frame = primary.read_accumulator(1)
    finally:
        for t in trs:
            t.Close()
    for k in range(3):
        assert (blocks[k][..., 3] > 0).mean() > 0.3
        assert np.array_equal(bits(frame[30 * k:30 * (k + 1)]), bits(blocks[k])), k


def test_renderer_frame_carries_the_blocks_moments(host):
    """The C++ frame loop with three tracers: polaris_host_renderer_set_variance turns the moments on in every tracer, and each
    pixel's .w is then a sum of L^2 of its own block: >= (sum L)^2 / n, 0 exactly where no sample saw light, and no band left empty;
    without, .w is 0.  The renderer does not expose its tracers' trace accumulators, and which tracer draws which seeds follows the
    worker threads' order, so exact equality with each block's .w is checked by the frame loop by hand above
    (test_three_block_frame_equals_each_blocks_trace_accumulator), not here."""
    from polaris_amd import scenes

    sc = scenes.SCENES["cornell"]()
    W, H, spp = 96, 90, 8
    acc = {}
    for on in (False, True):
        r = host.Renderer(sc, [0, 0, 0], primary=1, width=W, height=H, spp=spp, seed=3)
        try:
            if on:
                r.set_variance(**VA)
            rows, _ = r.render()
            _, acc[on] = r.read()
        finally:
            r.close()
        assert rows == [30, 30, 30]
    assert np.all(bits(acc[False][..., 3]) == 0)
    w, L = acc[True][..., 3].astype(np.float64), VO.lum(acc[True][..., :3]).astype(np.float64)
    assert np.all(w >= L * L / spp * (1 - 1e-5) - 1e-30)
    assert np.array_equal(w == 0, L == 0)
    assert (w.reshape(3, 30, W).mean(axis=(1, 2)) > 0).all()


# ---- 5. exact mode ----------------------------------------------------------------------------------------------------------------
def test_exact_mode_refuses_moments_in_both_orders(built):
    from polaris_amd import scenes
    from polaris_amd.tracer import TracerError as PolarisError

    sc = scenes.SCENES["cornell"]()
    for first, second in (("exact_accumulate", "moments"), ("moments", "exact_accumulate")):
        tr = make_hip_tracer(sc, 32, 32)
        try:
            tr.set_option(first, 1)
            with pytest.raises(PolarisError) as e:
                tr.set_option(second, 1)
            assert e.value.code == 6                                   # POLARIS_E_UNSUPPORTED
        finally:
            tr.Close()


def test_variance_needs_moments_and_aov_errors(built):
    from polaris_amd import scenes
    from polaris_amd.tracer import TracerError as PolarisError

    sc = scenes.SCENES["cornell"]()
    tr = make_hip_tracer(sc, 32, 32)
    try:
        p = T.variance_params(**VA)
        assert tr._lib.polaris_hip_set_variance(tr._h, T.C.byref(p)) == 2   # moments off: POLARIS_E_BAD_ARGUMENT
        with pytest.raises(PolarisError):
            tr.read_aov(T.AOV_VARIANCE)
        tr.set_variance(**VA)
        with pytest.raises(PolarisError):
            tr.read_aov(T.AOV_VARIANCE)                                # before any variance sync
        with pytest.raises(PolarisError):
            tr.set_option("moments", 0)
        for bad in (dict(sigma_variance=-1.0), dict(sigma_variance=1e7), dict(min_samples=0), dict(min_samples=65)):
            with pytest.raises(PolarisError):
                tr.set_variance(**{**VA, **bad})
        tr.set_variance(0.0)
        tr.set_option("moments", 0)
    finally:
        tr.Close()


# ---- 6. caller planes against the CPU restatement ---------------------------------------------------------------------------------
SHAPES = [(61, 37, 0, None), (300, 9, 0, None), (97, 61, 13, 29), (257, 20, 19, 1), (1, 40, 0, None), (40, 1, 0, None), (64, 64, 31, 2),
          (33, 65, 64, 1), (128, 96, 0, 50)]
PARAMS = [dict(iterations=4, normal_power_log2=5, sigma_depth=0.1, sigma_variance=4.0, min_samples=4),
          dict(iterations=5, normal_power_log2=7, sigma_depth=0.1, sigma_variance=1.0, min_samples=2),
          dict(iterations=2, normal_power_log2=0, sigma_depth=0.0, sigma_variance=8.0, min_samples=64),
          dict(iterations=8, normal_power_log2=10, sigma_depth=2.0, sigma_variance=0.5, min_samples=1),
          dict(iterations=0, normal_power_log2=5, sigma_depth=0.1, sigma_variance=4.0, min_samples=4),
          dict(iterations=1, normal_power_log2=3, sigma_depth=0.5, sigma_variance=1e-6, min_samples=8),
          dict(iterations=3, normal_power_log2=5, sigma_depth=0.1, sigma_variance=1e6, min_samples=16),
          dict(iterations=4, normal_power_log2=1, sigma_depth=1.0, sigma_variance=2.0, min_samples=3)]


def plane_cases(W, H, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for s in (1, 3, 16):
        cases.append((f"random{s}", s) + VO.moment_planes(rng, H, W, s))
    acc, g, a = VO.flat_planes(H, W, 8)
    acc[..., :3] = 0.5
    acc[..., 3] = VO.lum(acc[..., :3] / 8) ** 2 * 8                     # v = 0 everywhere
    acc[: H // 2, :, :3] = 1.0
    cases.append(("v0", 8, acc, g, a))
    acc, g, a = VO.moment_planes(rng, H, W, 2)
    a[..., :3][rng.random((H, W, 3)) < 0.2] = 0.0
    a[..., 3][rng.random((H, W)) < 0.2] = G.leaf_word(-1)
    a[..., 3][rng.random((H, W)) < 0.1] = G.leaf_word(T.BXDF_EMISSIVE)
    cases.append(("misses", 2, acc, g, a))
    return cases


@pytest.mark.parametrize("W,H,block_y,block_h", SHAPES)
def test_variance_planes_bit_equal_to_cpu(host, oracle, W, H, block_y, block_h):
    from polaris_amd.tracer import HipTracer

    bh = H - block_y if block_h is None else block_h
    rows = slice(block_y, block_y + bh)
    outside = np.ones(H, bool)
    outside[rows] = False
    tr = HipTracer("planes", 0)
    tr.Init()
    try:
        for pi, p in enumerate(PARAMS):
            for name, s, acc, g, a in plane_cases(W, H, 100 * pi + W + H):
                rng = np.random.default_rng(pi)
                pre_v = rng.random((H, W, 4), dtype=np.float32)
                pre_d = rng.random((H, W, 4), dtype=np.float32)
                pre_fb = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
                var, den, fb = tr.variance_planes(acc, g, a, samples=s, exposure=1.2, block_y=block_y, block_h=block_h, variance=pre_v,
                                                  denoised=pre_d, rgba=pre_fb, **p)
                kw = dict(normal_power_log2=p["normal_power_log2"], sigma_depth=p["sigma_depth"], sigma_variance=p["sigma_variance"],
                          min_samples=p["min_samples"])
                want_v = host.variance(acc, s, g, a, block_y=block_y, block_h=block_h, **kw)
                tag = (name, pi)
                assert np.array_equal(bits(var[rows]), bits(want_v[rows])), tag
                assert np.array_equal(bits(var[outside]), bits(pre_v[outside])), tag
                assert np.array_equal(fb[outside], pre_fb[outside]), tag
                w = F(1.0 / float(F(s)))
                if p["iterations"]:
                    want_d = host.denoise_variance(acc, w, want_v, g, a, block_y=block_y, block_h=block_h, iterations=p["iterations"], **kw)
                    assert np.array_equal(bits(den[rows]), bits(want_d[rows])), tag
                    assert np.array_equal(bits(den[outside]), bits(pre_d[outside])), tag
                    want_fb = oracle.tonemap(want_d, 1.0, 1.2).reshape(H, W, 4)
                else:
                    assert np.array_equal(bits(den), bits(pre_d)), tag
                    want_fb = oracle.tonemap(acc, float(w), 1.2).reshape(H, W, 4)
                assert np.array_equal(fb[rows], want_fb[rows]), tag
    finally:
        tr.Close()


# ---- 7. the real path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp,block", [(4, (0, None)), (64, (0, None)), (4, (13, 21))])
def test_real_path_matches_host_chain(host, oracle, spp, block):
    from polaris_amd import scenes

    W, H = 96, 72
    by, bh = block
    rows = slice(by, H if bh is None else by + bh)
    sc = scenes.SCENES["cornell"](W / H)
    tr = make_hip_tracer(sc, W, H)
    try:
        tr.set_denoise(**DN)
        tr.set_variance(**VA)
        trace(tr, W, H, spp, base=3)
        sync(tr, W, H, spp, block_y=by, block_h=bh)
        got = {k: tr.read_aov(k) for k in (T.AOV_VARIANCE, T.AOV_DENOISED, T.AOV_GUIDE, T.AOV_ALBEDO)}
        acc, fb = tr.read_accumulator(1), tr.read_framebuffer()
    finally:
        tr.Close()
    g, a = got[T.AOV_GUIDE], got[T.AOV_ALBEDO]
    kw = dict(normal_power_log2=DN["normal_power_log2"], sigma_depth=DN["sigma_depth"], **VA)
    var = host.variance(acc, spp, g, a, block_y=by, block_h=bh, **kw)
    den = host.denoise_variance(acc, F(1.0 / float(F(spp))), var, g, a, block_y=by, block_h=bh, iterations=DN["iterations"], **kw)
    assert np.array_equal(bits(got[T.AOV_VARIANCE][rows]), bits(var[rows]))
    assert np.array_equal(bits(got[T.AOV_DENOISED][rows]), bits(den[rows]))
    assert (var[rows][..., 3] > 0).mean() > 0.3
    assert np.array_equal(fb[rows], oracle.tonemap(den, 1.0, 1.2).reshape(H, W, 4)[rows])


def test_real_path_with_temporal_reuse_matches_host_chain(host, oracle):
    from polaris_amd import scenes

    W, H, spp = 96, 72, 4
    sc0 = scenes.SCENES["cornell"](W / H)
    sc1 = moved(sc0, 0.02, 0.01)
    tp = T.TEMPORAL_DEFAULTS
    kw = dict(normal_power_log2=DN["normal_power_log2"], sigma_depth=DN["sigma_depth"], **VA)
    tr = make_hip_tracer(sc0, W, H)
    try:
        tr.set_denoise(**DN)
        tr.set_temporal(**tp)
        tr.set_variance(**VA)
        trace(tr, W, H, spp, base=3)
        sync(tr, W, H, spp)
        hist, hvar, g0, a0 = (tr.read_aov(k) for k in (T.AOV_TEMPORAL, T.AOV_VARIANCE, T.AOV_GUIDE, T.AOV_ALBEDO))
        acc0 = tr.read_accumulator(1)
        from polaris_amd.tracer import ChangeType, UpdateMode

        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc1)
        trace(tr, W, H, spp, base=5)
        sync(tr, W, H, spp)
        got = {k: tr.read_aov(k) for k in (T.AOV_PRIOR, T.AOV_PRIOR2, T.AOV_TEMPORAL, T.AOV_VARIANCE, T.AOV_DENOISED, T.AOV_GUIDE,
                                           T.AOV_ALBEDO)}
        acc = tr.read_accumulator(1)
    finally:
        tr.Close()
    assert np.array_equal(bits(hvar), bits(host.variance(acc0, spp, g0, a0, temporal=hist, prior2=np.zeros_like(hist), **kw)))
    g1, a1 = got[T.AOV_GUIDE], got[T.AOV_ALBEDO]
    prior, prior2 = host.reproject_moments(hist, hvar, g0, a0, sc0.eye, sc0.frustum, g1, a1, sc1.eye, sc1.frustum, **tp)
    assert (prior2[..., 3] > 0).mean() > 0.5
    assert np.array_equal(bits(got[T.AOV_PRIOR]), bits(prior))
    assert np.array_equal(bits(got[T.AOV_PRIOR2]), bits(prior2))
    tmp = host.temporal_combine(acc, prior, 0, spp)
    assert np.array_equal(bits(got[T.AOV_TEMPORAL]), bits(tmp))
    var = host.variance(acc, spp, g1, a1, temporal=tmp, prior2=prior2, **kw)
    assert np.array_equal(bits(got[T.AOV_VARIANCE]), bits(var))
    assert (var[..., 2] > spp).mean() > 0.5                                  # n_eff = n + m
    den = host.denoise_variance(tmp, F(1), var, g1, a1, iterations=DN["iterations"], **kw)
    assert np.array_equal(bits(got[T.AOV_DENOISED]), bits(den))


# ---- 8. invariants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["variance_denoise_off", "sigma_zero_denoise_on"])
def test_frame_buffer_bytes_unchanged(built, mode):
    from polaris_amd import scenes

    W, H = 80, 64
    sc = scenes.SCENES["cornell"](W / H)
    out = {}
    for on in (False, True):
        tr = make_hip_tracer(sc, W, H)
        try:
            if mode == "sigma_zero_denoise_on":
                tr.set_denoise(**DN)
                if on:
                    tr.set_option("moments", 1)
                    tr.set_variance(0.0)
            elif on:
                tr.set_variance(**VA)
            trace(tr, W, H, 4, base=3)
            sync(tr, W, H, 4)
            trace(tr, W, H, 4, base=4, accumulated=4)
            sync(tr, W, H, 4, accumulated=4, block_y=10, block_h=30)
            out[on] = tr.read_framebuffer()
            if on and mode == "variance_denoise_off":
                assert tr.read_aov(T.AOV_VARIANCE)[10:40, :, 2].min() == 8
        finally:
            tr.Close()
    assert np.array_equal(out[False], out[True])


@pytest.mark.parametrize("drop", ["max_history", "resize", "upload"])
def test_moment_history_is_dropped(built, drop):
    from polaris_amd import scenes
    from polaris_amd.tracer import ChangeType, UpdateMode
    from polaris_amd.tracer import TracerError as PolarisError

    W, H = 64, 48
    sc0 = scenes.SCENES["cornell"](W / H)
    sc1 = moved(sc0, 0.02)
    tr = make_hip_tracer(sc0, W, H)
    try:
        tr.set_temporal()
        tr.set_variance(**VA)
        trace(tr, W, H, 4, base=3)
        sync(tr, W, H, 4)
        if drop == "max_history":
            tr.set_temporal(0)
            tr.set_temporal()
        elif drop == "resize":
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, (W, H))
        else:
            tr.UpdateState(UpdateMode.Synchronous, ChangeType.SceneData, sc0)
        with pytest.raises(PolarisError):
            tr.read_aov(T.AOV_VARIANCE) if drop == "resize" else tr.read_aov(T.AOV_PRIOR2)
        tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc1)
        trace(tr, W, H, 4, base=5)
        sync(tr, W, H, 4)
        prior2, var = tr.read_aov(T.AOV_PRIOR2), tr.read_aov(T.AOV_VARIANCE)
    finally:
        tr.Close()
    assert np.all(bits(prior2) == 0)
    assert np.all(var[..., 2] == 4)                                          # no history: n_eff = n


# ---- 9. quality on the device -----------------------------------------------------------------------------------------------------
def test_quality_on_the_device(built):
    """512^2 layered box against 256 spp: (a) at 4 spp the guided filter is no worse than today's; (b) at 64 spp it is no worse than
    the unfiltered mean."""
    from polaris_amd import scenes

    N = 512
    sc = scenes.SCENES["cornell"]()
    res = {}
    for spp, base in ((256, 99), (4, 11), (64, 21)):
        for mode in (("plain", "old", "var") if spp != 256 else ("plain",)):
            tr = make_hip_tracer(sc, N, N)
            try:
                if mode != "plain":
                    tr.set_denoise(**DN)
                if mode == "var":
                    tr.set_variance(**VA)
                trace(tr, N, N, spp, base=base)
                sync(tr, N, N, spp)
                a = tr.read_aov(T.AOV_ALBEDO)
                res[(spp, mode)] = (tr.read_accumulator(1)[..., :3] / spp if mode == "plain" else tr.read_aov(T.AOV_DENOISED)[..., :3], a)
            finally:
                tr.Close()
    want, a = res[(256, "plain")]
    filt = G.filtered_mask(a)
    rmse = lambda x: float(np.sqrt(np.mean((x[filt] - want[filt]) ** 2)))  # noqa: E731
    r4 = {m: rmse(res[(4, m)][0]) for m in ("plain", "old", "var")}
    r64 = {m: rmse(res[(64, m)][0]) for m in ("plain", "old", "var")}
    print(f"device quality 512^2 layered: 4 spp {r4}; 64 spp {r64}")
    assert r4["var"] <= r4["old"], r4
    assert r64["var"] <= r64["plain"], r64
