"""The test entries that work on caller planes, on the MI355X (include/polaris_hip.h: polaris_hip_reproject_planes,
_reproject_motion_planes, _reproject_deform_planes; _display_planes, _bloom_planes, _denoise_planes, _variance_planes).  The three
reprojection entries are one body over one description (polaris_amd/csrc/reproject_io.h) whose rules the CPU restatements share.

Bars: the device entries agree with each other bit for bit where tests/test_vertex_motion_cpu.py and tests/test_motion_cpu.py say
the host entries do -- unchanged vertices give object motion's planes, two equal tables with one shared INSTANCE word give the
camera-only PRIOR (and polaris_host_reproject_moments' PRIOR2) -- and each call runs the kernel variant its groups select; every
violation of tests/reproject_args.py that applies to a device entry is refused with POLARIS_E_BAD_ARGUMENT, launches nothing, and
the valid call straight after it still equals the host; the four other entries refuse rows outside the frame and leave the rows
outside a request as they were passed."""
import numpy as np
import pytest

import motion_oracle as MO
import reproject_args as RA
import variance_oracle as VA
import vertex_motion_oracle as VO
from conftest import bits
from polaris_amd import ctypes_api as T

pytestmark = pytest.mark.gpu

F = np.float32
TP = T.TEMPORAL_DEFAULTS
PLAIN, MOTION, MOTION_M2 = "pol::k_reproject<false, false>", "pol::k_reproject<false, true>", "pol::k_reproject<true, true>"
DEFORM, DEFORM_M2 = "pol::k_reproject_deform<false>", "pol::k_reproject_deform<true>"


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


@pytest.fixture(scope="module")
def tr(built):
    from polaris_amd.tracer import HipTracer

    t = HipTracer("entries", 0)
    t.Init()
    t.set_option("time_kernels", 1)
    yield t
    t.Close()


def same(got, want):
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    return len(got) == len(want) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))


def plain_args(a):
    return a[:3] + a[4:8] + a[9:11]                # (MO.ORDER without the INSTANCE planes and the tables)


# ---- 1. the entries against each other ------------------------------------------------------------------------------------------
def test_entries_agree_where_the_host_entries_do(tr, host):
    W, H, nt = 32, 24, 16
    rng = np.random.default_rng(3)
    for name, c in MO.engineered_cases(W, H):
        a = MO.args(c)
        # unchanged vertices: object motion's planes, whatever the HIT plane's triangle (inside the scene) and barycentrics say
        verts = np.zeros((3 * nt, 4), F)
        verts[:, :3] = rng.standard_normal((3 * nt, 3)).astype(F)
        verts[5, 1], verts[7, 2] = np.nan, F(-0.0)                     # (equal bytes, whatever they spell)
        hit = VO.hit_plane(rng.integers(0, nt, (H, W)), rng.random((H, W)).astype(F), rng.random((H, W)).astype(F))
        motion = tr.reproject_motion_planes(*a, **TP)
        assert tr.kernel_symbol("reproject") == MOTION
        deform = tr.reproject_deform_planes(*a, hit, verts, verts.copy(), **TP)
        assert tr.kernel_symbol("reproject") == DEFORM
        assert same(deform, motion), name
        motion2 = tr.reproject_motion_planes(*a, history_variance=c["hvar"], **TP)
        assert tr.kernel_symbol("reproject") == MOTION_M2
        deform2 = tr.reproject_deform_planes(*a, hit, verts, verts.copy(), history_variance=c["hvar"], **TP)
        assert tr.kernel_symbol("reproject") == DEFORM_M2
        assert len(deform2) == 2 and same(deform2, motion2), name + " (M2)"
        assert same(motion, host.reproject_motion(*a, **TP)) and same(motion2, host.reproject_motion(*a, history_variance=c["hvar"], **TP)), name
        # two equal tables and one shared INSTANCE word: the camera-only reprojection
        plain = tr.reproject_planes(*plain_args(a), **TP)
        assert tr.kernel_symbol("reproject") == PLAIN
        want, want2 = host.reproject_moments(a[0], c["hvar"], *plain_args(a)[1:], **TP)
        assert same(plain, want), name
        for word in (0, 1):
            inst = np.full((H, W), word, np.uint32)
            still = a[:3] + [inst] + a[4:8] + [inst] + a[9:11] + [c["pt"], c["pt"].copy()]
            assert same(tr.reproject_motion_planes(*still, **TP), plain), (name, word)
            assert tr.kernel_symbol("reproject") == MOTION
            assert same(tr.reproject_motion_planes(*still, history_variance=c["hvar"], **TP), (plain, want2)), (name, word, "M2")
            assert tr.kernel_symbol("reproject") == MOTION_M2
        if name == "translated":
            assert (plain[..., 3] > 0).mean() > 0.3 and (motion[c["i"] == 1, 3] > 0).mean() > 0.3


# ---- 2. the refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,moments", [("reproject", False), ("reproject_motion", False), ("reproject_motion", True),
                                           ("reproject_deform", False), ("reproject_deform", True)])
def test_device_entries_refuse_what_the_host_entries_refuse(tr, host, entry, moments):
    from polaris_amd.tracer import TracerError

    fn = getattr(tr._lib, "polaris_hip_" + RA.DEVICE[entry])

    def device(d):
        tr._check(RA.raw(fn, entry, d, tr._h), tr._h)
        return (d["prior"], d["prior2"]) if moments else d["prior"]

    d = RA.valid(entry, moments)
    assert RA.raw(getattr(host.load(), "polaris_host_" + entry), entry, d) == 0
    want = (d["prior"].copy(), d["prior2"].copy()) if moments else d["prior"].copy()
    assert (d["prior"][..., 3] > 0).sum() >= 8
    assert same(device(RA.valid(entry, moments)), want)
    rows = RA.rows(entry)
    assert len(rows) >= 23
    for name, change in rows:
        tr.kernel_ms("reproject")                                      # (reading a timer clears it)
        with pytest.raises(TracerError) as e:
            device(RA.violated(entry, change, moments))
        assert e.value.code == RA.BAD_ARGUMENT and RA.DEVICE[entry] + ":" in str(e.value), (name, str(e.value))
        assert tr.kernel_ms("reproject")[1] == 0, name                 # nothing was launched
        assert same(device(RA.valid(entry, moments)), want), name      # ... and the next call is as good as ever
        assert tr.kernel_ms("reproject")[1] == 1


# ---- 3. the two smaller families -------------------------------------------------------------------------------------------------
def test_row_rules_of_the_other_plane_entries(tr, host):
    """display_planes, bloom_planes, denoise_planes and variance_planes on an 8 x 4 frame: rows [3, +2) leave the frame and are refused;
    rows [1, +2) are the host's bit for bit, and rows 0 and 3 come back as passed."""
    from polaris_amd.tracer import TracerError

    W, H, by, bh = 8, 4, 1, 2
    rows = slice(by, by + bh)
    outside = np.ones(H, bool)
    outside[rows] = False
    rng = np.random.default_rng(5)
    acc, g, a = VA.moment_planes(rng, H, W, 4)
    plane = (rng.random((H, W, 4)) * 2).astype(F)
    pre = {k: rng.random((H, W, 4), dtype=F) for k in ("variance", "denoised")}
    fb0 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    dn = dict(T.DENOISE_DEFAULTS)
    va = dict(normal_power_log2=dn["normal_power_log2"], sigma_depth=dn["sigma_depth"], **T.VARIANCE_DEFAULTS)
    calls = {
        "display_planes": lambda **r: tr.display_planes(plane, rgba=fb0, auto_exposure=1, **r)[:1],
        "bloom_planes": lambda **r: tr.bloom_planes(plane, rgba=fb0, **r, **T.BLOOM_DEFAULTS)[:1],
        "denoise_planes": lambda **r: tr.denoise_planes(acc, g, a, weight=F(0.25), exposure=1.2, denoised=pre["denoised"], rgba=fb0, **r, **dn)[::-1],
        "variance_planes": lambda **r: tr.variance_planes(acc, g, a, samples=4, exposure=1.2, variance=pre["variance"], denoised=pre["denoised"],
                                                          rgba=fb0, iterations=dn["iterations"], **r, **va)[::-1],
    }
    want = {
        "display_planes": (host.display(plane, rgba=fb0, auto_exposure=1, block_y=by, block_h=bh)[0],),
        "bloom_planes": (host.bloom(plane, rgba=fb0, block_y=by, block_h=bh, **T.BLOOM_DEFAULTS)[0],),
        "denoise_planes": (None, host.denoise(acc, F(0.25), g, a, block_y=by, block_h=bh, out=pre["denoised"], **dn)),
    }
    want_v = host.variance(acc, 4, g, a, block_y=by, block_h=bh, out=pre["variance"], **va)
    want["variance_planes"] = (None, host.denoise_variance(acc, F(1.0 / float(F(4))), want_v, g, a, block_y=by, block_h=bh, out=pre["denoised"],
                                                           iterations=dn["iterations"], **va), want_v)
    for name, call in calls.items():
        with pytest.raises(TracerError) as e:
            call(block_y=3, block_h=2)
        assert e.value.code == RA.BAD_ARGUMENT and name + ":" in str(e.value), str(e.value)
        got = call(block_y=by, block_h=bh)                              # (RGBA8 first, then the float planes)
        assert np.array_equal(got[0][outside], fb0[outside]) and not np.array_equal(got[0][rows], fb0[rows]), name
        assert len(got) == len(want[name])
        for x, y in zip(got, want[name]):
            assert y is None or np.array_equal(bits(x), bits(y)), name
