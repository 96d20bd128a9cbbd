"""Temporal reuse across moving mesh instances on the CPU (no GPU; option "object_motion"): the motion matrix
and polaris_host_reproject_motion -- the restatement tests/test_gpu_motion.py compares the kernels with bit for bit -- against an
independent numpy statement (tests/motion_oracle.py), the rigid-motion property, and the quality the feature exists for."""
import dataclasses

import numpy as np
import pytest

import gbuffer_oracle as G
import motion_oracle as MO
import test_temporal_cpu as TC
from polaris_amd import ctypes_api as T

F = np.float32
DEFAULTS = T.TEMPORAL_DEFAULTS
DELTA = (0.1, 0.05, 0.2)


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    return host_api


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. the motion matrix ----------------------------------------------------------------------------------------------------
def matrices():
    from polaris_amd import scenes as S

    rng = np.random.default_rng(4)
    ms = [np.eye(4), S.translation((0.3, -2.0, 5.5)), S.translation((1e-3, 0, 0)), S.rotation_y(0.05), S.rotation_y(-2.4),
          S.scaling(1.0, 1.6, 0.7), S.scaling(0.05, 3.0, 12.0), S.translation((1, 2, 3)) @ S.rotation_y(0.6) @ S.scaling(1.0, 1.6, 0.7)]
    ms += [S.translation(rng.standard_normal(3)) @ S.rotation_y(rng.uniform(-3, 3)) @ S.scaling(*rng.uniform(0.3, 3, 3)) for _ in range(4)]
    ti = S.transformed_instances().mesh_instances["inv_transform"]
    assert len(ti) == 6
    return [MO.inv16(m) for m in ms] + [np.asarray(m, F) for m in ti]


def test_motion_matrix_against_numpy(host):
    table = matrices()
    moved = 0
    for a in table:
        for b in table:
            flag, D = host.motion_matrix(a, b)
            wflag, wD = MO.motion(a, b)
            assert flag == wflag
            if flag == MO.STATIC:
                assert a.tobytes() == b.tobytes() and np.array_equal(D, np.eye(4, dtype=F)[:3])
                continue
            moved += 1
            assert flag == MO.MOVED
            # 1e-6 relative, the 3 x 3 and the translation column each to its own largest entry (a translation of 5 must not hide an
            # error in a rotation's entries); float32 rounding of the result alone is 6e-8
            assert np.abs(D[:, :3] - wD[:, :3]).max() <= 1e-6 * np.abs(wD[:, :3]).max(), (a, b)
            assert np.abs(D[:, 3] - wD[:, 3]).max() <= 1e-6 * max(np.abs(wD[:, 3]).max(), 1e-30), (a, b)
    assert moved == sum(a.tobytes() != b.tobytes() for a in table for b in table) >= len(table) * (len(table) - 2)


def test_motion_matrix_static_and_invalid(host):
    a = matrices()[7]
    assert host.motion_matrix(a, a.copy())[0] == MO.STATIC
    b = a.copy()
    b[13] = np.nextafter(b[13], F(9))                               # one ulp in the translation: no longer byte-equal
    flag, D = host.motion_matrix(a, b)
    assert flag == MO.MOVED and np.abs(D - np.eye(4)[:3]).max() < 1e-5
    nz = a.copy()
    nz[0] = F(-0.0) if a[0] == 0 else a[0]
    for col in range(3):                                             # a zero column, in the history's matrix or the current one
        z = a.copy()
        z[4 * col:4 * col + 4] = 0
        for pair in ((z, a), (a, z)):
            flag, D = host.motion_matrix(*pair)
            assert flag == MO.INVALID and np.all(D == 0)
    for bad in (np.inf, np.nan):
        z = a.copy()
        z[5] = bad
        assert host.motion_matrix(z, a)[0] == MO.INVALID and host.motion_matrix(a, z)[0] == MO.INVALID
    big = MO.inv16(np.diag([1e-30, 1e-30, 1e-30, 1.0]))             # D = inverse(Inv_hist) . Inv_cur overflows float32
    small = MO.inv16(np.diag([1e30, 1e30, 1e30, 1.0]))
    assert host.motion_matrix(small, big)[0] == MO.INVALID


# ---- the rigid pair: one Cornell-diffuse instance translated by DELTA, the camera with it --------------------------------------
@pytest.fixture(scope="module")
def rigid(oracle):
    from polaris_amd import scenes as S

    W = H = 64
    sc0 = S.cornell_box("diffuse")
    sc1 = S.cornell_box("diffuse", world=S.translation(DELTA))
    follow = dataclasses.replace(sc1, eye=(np.asarray(sc1.eye, F) + np.asarray(DELTA, F)).astype(F))
    beside = dataclasses.replace(sc1, eye=(np.asarray(follow.eye, F) + np.array([0.013, 0.007, 0], F)).astype(F))
    gy, gx = np.mgrid[0:H, 0:W] / 16.0
    hist = np.zeros((H, W, 4), F)
    hist[..., 0], hist[..., 1], hist[..., 2] = 1 + 0.5 * np.sin(gx), 1 + 0.5 * np.cos(gy), 0.5 + 0.1 * gx * gy
    hist[..., 3] = 24 + 8 * np.sin(gx + gy)
    return dict(W=W, H=H, hist=hist, sc0=sc0, p0=MO.gbuffer_inst(oracle, sc0, W, H), follow=follow, p_follow=MO.gbuffer_inst(oracle, follow, W, H),
                beside=beside, p_beside=MO.gbuffer_inst(oracle, beside, W, H))


def rigid_args(r, which):
    sc0, sc1 = r["sc0"], r[which]
    (pg, pa, pi), (g, a, i) = r["p0"], r["p_" + which]
    return [r["hist"], pg, pa, pi, sc0.eye, sc0.frustum, g, a, i, sc1.eye, sc1.frustum, MO.inv_table(sc0), MO.inv_table(sc1)]


# ---- 2. the restatement against the independent statement ----------------------------------------------------------------------
def test_restatement_matches_independent_statement_on_the_rigid_pair(host, rigid):
    """polaris_host_reproject_motion against the numpy statement to 1e-5 on the planes of the rigid property (`follow`), over every
    filtered pixel, m included.  The projected points fall on the history's pixel centres there, where a float32 and a float64 floor
    may pick different 2 x 2 taps -- but the tap that differs has a weight of ~1e-6, so the PRIOR is continuous across it and the
    position is left out of the margin; only pixels with a tap within 1e-4 of its normal or depth threshold are left out.  Measured:
    3760 of 3760 filtered pixels compared (100 %), largest difference 3.0e-7 relative.  Then the same with the current camera a
    little beside the translated one, so that the points fall between the centres (there the position stays in the margin)."""
    a = rigid_args(rigid, "follow")
    filt = G.filtered_mask(rigid["p_follow"][1])
    got = host.reproject_motion(*a, **DEFAULTS)
    want, margin = MO.reproject_motion(*a, position_margin=False, **DEFAULTS)
    sure = filt & (margin > 1e-4)
    print(f"rigid pair: {int(sure.sum())} of {int(filt.sum())} filtered pixels compared, max relative difference "
          f"{np.max(np.abs(got[sure] - want[sure]) / np.maximum(np.abs(want[sure]), 1)):.2e}")
    assert sure.sum() == filt.sum()
    assert np.array_equal(got[sure, 3] > 0, want[sure, 3] > 0)
    np.testing.assert_allclose(got[sure], want[sure], rtol=1e-5, atol=1e-5)
    assert np.all(got[~filt] == 0) and np.all(want[~filt] == 0)
    a = rigid_args(rigid, "beside")
    got = host.reproject_motion(*a, **DEFAULTS)
    want, margin = MO.reproject_motion(*a, **DEFAULTS)
    sure = margin > 1e-4
    assert sure.mean() > 0.7 and (got[sure, 3] > 0).mean() > 0.8
    np.testing.assert_allclose(got[sure], want[sure], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("W,H", [(64, 48), (37, 53)])
def test_restatement_matches_independent_statement_on_engineered_instances(host, W, H):
    for name, c in MO.engineered_cases(W, H):
        gy, gx = np.mgrid[0:H, 0:W] / 16.0                              # (a smooth history, holes kept: see test_temporal_cpu)
        holes = c["hist"][..., 3] == 0
        c["hist"][..., 0], c["hist"][..., 1], c["hist"][..., 2] = 1 + 0.5 * np.sin(gx), 1 + 0.5 * np.cos(gy), 0.5 + 0.1 * gx * gy
        c["hist"][..., 3] = np.where(holes, 0, 24 + 8 * np.sin(gx + gy))
        c["hvar"][..., 1] = 0.3 + 0.1 * np.cos(gx - gy)              # (the history's M2, smooth too)
        got, got2 = host.reproject_motion(*MO.args(c), history_variance=c["hvar"], **DEFAULTS)
        want, want2, margin = MO.reproject_motion(*MO.args(c), history_variance=c["hvar"], **DEFAULTS)
        assert np.array_equal(bits(got), bits(host.reproject_motion(*MO.args(c), **DEFAULTS)))   # (PRIOR does not depend on M2)
        sure = margin > 1e-4
        filt = G.filtered_mask(c["a"])
        assert sure[filt].mean() > (0.3 if name == "invalid" else 0.6), name
        np.testing.assert_allclose(got[sure], want[sure], rtol=1e-5, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(got2[sure], want2[sure], rtol=1e-5, atol=1e-5, err_msg=name + " PRIOR2")
        assert np.all(got2[..., 1:3] == 0) and np.array_equal(got2[..., 3], got[..., 3])
        assert np.all(got[~filt] == 0)
        box = filt & (c["i"] == 1)
        if name == "invalid":
            assert box.any() and np.all(got[box] == 0)
        elif name in ("translated", "rotation+scale", "static"):
            assert (got[box, 3] > 0).mean() > 0.5, name               # the box's pixels find their history through D
            assert (got2[box, 0] > 0).mean() > 0.5, name              # ... and its M2
        if name == "miss words":
            assert np.all(got[c["i"] >= 2] == 0)


# ---- 3. it reduces to today's reprojection --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", [0.25, 0.05])
@pytest.mark.parametrize("m2", [False, True])
def test_reduces_to_the_camera_only_reprojection(host, dx, m2):
    rng = np.random.default_rng(21)
    pe, pf, pg, pa, e, f, g, a = TC.room_pair(dx=dx)
    H, W = g.shape[:2]
    hist = TC.history_planes(rng, H, W)
    hvar = (rng.random((H, W, 4)) * 2).astype(F)
    table = np.stack([MO.inv16(np.eye(4)), matrices()[9]])
    for word in (0, 1):
        inst = np.full((H, W), word, np.uint32)
        if m2:
            got, got2 = host.reproject_motion(hist, pg, pa, inst, pe, pf, g, a, inst, e, f, table, table.copy(), history_variance=hvar, **DEFAULTS)
            want, want2 = host.reproject_moments(hist, hvar, pg, pa, pe, pf, g, a, e, f, **DEFAULTS)
            assert np.array_equal(bits(got2), bits(want2))
        else:
            got = host.reproject_motion(hist, pg, pa, inst, pe, pf, g, a, inst, e, f, table, table.copy(), **DEFAULTS)
            want = host.reproject(hist, pg, pa, pe, pf, g, a, e, f, **DEFAULTS)
        assert (want[..., 3] > 0).mean() > 0.3
        assert np.array_equal(bits(got), bits(want))


# ---- 4. the rigid property ----------------------------------------------------------------------------------------------------
def test_rigid_motion_of_scene_and_camera_finds_every_pixels_history(host, rigid):
    """The scene's one instance and the camera move by the same translation: the image is the same, so the PRIOR of a filtered pixel is
    the history at that pixel.  Measured on the restatement at 64 x 64: m > 0 at 100.00 % of the filtered pixels (3760 of 3760), the
    largest |h - history| 1.2e-7 of the plane's maximum; the share is asserted at that figure, rounded down to a whole per cent."""
    a = rigid_args(rigid, "follow")
    hist = rigid["hist"]
    got = host.reproject_motion(*a, **DEFAULTS)
    filt = G.filtered_mask(rigid["p_follow"][1])
    have = filt & (got[..., 3] > 0)
    share = have.sum() / filt.sum()
    err = np.abs(got[have, :3] - hist[have, :3]).max() / hist[..., :3].max()
    print(f"rigid: m > 0 at {100 * share:.2f} % of {int(filt.sum())} filtered pixels, max |h - history| = {err:.2e} of the maximum")
    assert share >= 1.00
    assert err <= 1e-3
    np.testing.assert_allclose(got[have, 3], np.minimum(hist[have, 3], DEFAULTS["max_history"]), atol=2e-2)
    assert np.all(got[~filt] == 0)
    # the camera-only arithmetic on the same planes looks DELTA away: it must not find the same history
    plain = host.reproject(*a[:3], *a[4:8], *a[9:11], **DEFAULTS)
    off = filt & (plain[..., 3] > 0)
    assert off.sum() < 0.5 * filt.sum() or np.abs(plain[off, :3] - hist[off, :3]).max() / hist[..., :3].max() > 1e-2


def test_malformed_arguments_are_rejected(host):
    name, c = MO.engineered_cases(16, 12)[1]
    a = MO.args(c)
    host.reproject_motion(*a, **DEFAULTS)
    with pytest.raises(ValueError):
        host.reproject_motion(*a[:3], c["pi"][:4], *a[4:], **DEFAULTS)
    with pytest.raises(ValueError):
        host.reproject_motion(*a[:11], c["pt"], c["ct"][:1], **DEFAULTS)
    with pytest.raises(ValueError):
        host.reproject_motion(*a[:11], c["pt"][:0], c["ct"][:0], **DEFAULTS)
    with pytest.raises(ValueError):
        host.reproject_motion(*a, max_history=5000)


# ---- 5. quality -----------------------------------------------------------------------------------------------------------------
# Ratios recorded in profiles/motion_quality.txt, each guarded at measured x 1.1: the margin covers the seed noise of a
# 1 spp trace, nothing else.
ONE_MOVE = {"a/b all": 0.190, "a/c moved": 0.304}


def test_quality_one_move_and_eight(host, oracle):
    res = MO.quality_run(host, oracle, 8, report=(1, 8))
    one, eight = res[1], res[8]
    for k, r in res.items():
        print(f"step {k}: " + "  ".join(f"{s} {' '.join(f'{n} {v:.4f}' for n, v in r[s].items())}" for s in "abc") + f"  reused {r['reused']:.3f} pixels {r['pixels']}")
    assert one["reused"] > 0.5
    assert one["a"]["all"] <= one["b"]["all"]
    assert one["a"]["moved"] <= one["c"]["moved"]
    assert one["a"]["all"] / one["b"]["all"] <= ONE_MOVE["a/b all"] * 1.1
    assert one["a"]["moved"] / one["c"]["moved"] <= ONE_MOVE["a/c moved"] * 1.1
    assert eight["a"]["all"] <= eight["b"]["all"]
