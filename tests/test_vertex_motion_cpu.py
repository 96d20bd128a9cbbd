"""Temporal reuse across mesh deformation on the CPU (no GPU; option "vertex_motion"):
polaris_host_reproject_deform -- the restatement tests/test_gpu_vertex_motion.py compares the kernels with bit for bit -- against an
independent numpy statement (tests/vertex_motion_oracle.py), its bit equality with the rigid path where no vertex changed, a rigid
motion expressed as a deformation, the rule of the history's vertices (frame_sync.h) and the quality the feature exists for."""
import os
import subprocess

import numpy as np
import pytest

import gbuffer_oracle as G
import motion_oracle as MO
import temporal_oracle as TO
import vertex_motion_oracle as VO
from conftest import ROOT
from polaris_amd import ctypes_api as T

F = np.float32
DEFAULTS = T.TEMPORAL_DEFAULTS


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    return host_api


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. the restatement against the independent statement -----------------------------------------------------------------------
def test_restatement_matches_independent_statement_on_engineered_planes(host):
    """polaris_host_reproject_deform against the numpy statement to 1e-5 (test_motion_cpu.py's bar) at 32 x 24 with 3 instances and 16
    triangles, with and without M2, over every pixel none of whose tests comes within 1e-4 of its threshold; and every branch of the
    arithmetic is shown to be taken by the planes."""
    W, H = 32, 24
    seen = {}
    for name, c in VO.engineered_cases(W, H):
        gy, gx = np.mgrid[0:H, 0:W] / 8.0                              # (a smooth history, holes kept: see test_temporal_cpu)
        holes = c["hist"][..., 3] == 0
        c["hist"][..., 0], c["hist"][..., 1], c["hist"][..., 2] = 1 + 0.5 * np.sin(gx), 1 + 0.5 * np.cos(gy), 0.5 + 0.1 * gx * gy
        c["hist"][..., 3] = np.where(holes, 0, 24 + 8 * np.sin(gx + gy))
        c["hvar"][..., 1] = 0.3 + 0.1 * np.cos(gx - gy)
        got, got2 = host.reproject_deform(*VO.args(c), history_variance=c["hvar"], **DEFAULTS)
        want, want2, margin = VO.reproject_deform(*VO.args(c), history_variance=c["hvar"], **DEFAULTS)
        assert np.array_equal(bits(got), bits(host.reproject_deform(*VO.args(c), **DEFAULTS))), name   # (PRIOR does not depend on M2)
        sure = margin > 1e-4
        filt = G.filtered_mask(c["a"])
        print(f"{name}: {int((sure & filt).sum())} of {int(filt.sum())} filtered pixels compared, m > 0 at {int((got[..., 3] > 0).sum())}")
        assert sure[filt].mean() > 0.5, name
        np.testing.assert_allclose(got[sure], want[sure], rtol=1e-5, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(got2[sure], want2[sure], rtol=1e-5, atol=1e-5, err_msg=name + " PRIOR2")
        assert np.all(got2[..., 1:3] == 0) and np.array_equal(got2[..., 3], got[..., 3])
        assert np.all(got[~filt] == 0) and (~filt).sum() > 0
        tri, inst = c["hit"][..., 0], c["i"]
        inside = filt & (tri < VO.N_TRIS) & (inst < VO.N_INST)
        changed = np.zeros((H, W), bool)
        changed[inside] = VO.changed_triangles(c["v"], c["pv"])[tri[inside]]
        seen[name] = dict(got=got, filt=filt, inside=inside, changed=changed, inst=inst, tri=tri, c=c)
    have = lambda s, m: (s["got"][m, 3] > 0)  # noqa: E731
    d = seen["deformed"]
    for k in range(3):                                                # every instance shows changed and unchanged triangles, both with history
        for ch in (False, True):
            m = d["inside"] & (d["inst"] == k) & (d["changed"] == ch)
            assert m.sum() >= 4 and have(d, m).mean() > 0.5, (k, ch)
    assert (d["c"]["hit"][..., 0] == VO.NO_TRIANGLE).sum() > 0 and np.all(d["got"][d["c"]["hit"][..., 0] == VO.NO_TRIANGLE] == 0)   # misses
    u = seen["undeformed"]
    assert not u["changed"].any() and have(u, u["inside"]).mean() > 0.5
    s = seen["invalid now"]                                           # instance 2 INVALID in the motion table alone
    m2 = s["inside"] & (s["inst"] == 2)
    assert (m2 & ~s["changed"]).sum() >= 4 and not have(s, m2 & ~s["changed"]).any()
    assert have(s, m2 & s["changed"]).mean() > 0.5
    s = seen["invalid then"]                                          # ... and in the deformation table too
    m2 = s["inside"] & (s["inst"] == 2)
    assert m2.sum() >= 8 and not have(s, m2).any() and have(s, s["inside"] & (s["inst"] == 1)).mean() > 0.5
    s = seen["words outside"]
    out = s["filt"] & ~s["inside"]
    assert (s["filt"] & (s["tri"] >= VO.N_TRIS)).sum() >= 4 and (s["filt"] & (s["inst"] >= VO.N_INST)).sum() >= 4 and not have(s, out).any()
    s = seen["non-finite"]
    for t, lost in ((0, True), (8, True), (1, False), (9, False)):   # (their neighbours in the same quad keep theirs)
        m = s["inside"] & (s["tri"] == t)
        assert m.sum() >= 2 and (not have(s, m).any() if lost else have(s, m).any()), t
    s = seen["instance mismatch"]
    blk = np.zeros((H, W), bool)
    blk[H // 4 + 1:H // 2 - 1, W // 4 + 1:3 * W // 4 - 1] = True
    assert have(d, blk & d["inside"]).sum() > have(s, blk & s["inside"]).sum()


# ---- 2. bit equality with the rigid path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(64, 48), (37, 53)])
def test_unchanged_vertices_are_bit_equal_to_object_motion(host, W, H):
    """prev_vertices byte-equal to vertices: PRIOR and PRIOR2 are polaris_host_reproject_motion's, bit for bit, on test_motion_cpu.py's
    planes -- whatever the HIT plane's triangle (inside the scene) and barycentrics say."""
    rng = np.random.default_rng(3)
    nt = 16
    for name, c in MO.engineered_cases(W, H):
        verts = np.zeros((3 * nt, 4), F)
        verts[:, :3] = rng.standard_normal((3 * nt, 3)).astype(F)
        verts[5, 1], verts[7, 2] = np.nan, F(-0.0)                     # (equal bytes, whatever they spell)
        hit = VO.hit_plane(rng.integers(0, nt, (H, W)), rng.random((H, W)).astype(F), rng.random((H, W)).astype(F))
        got, got2 = host.reproject_deform(*MO.args(c), hit, verts, verts.copy(), history_variance=c["hvar"], **DEFAULTS)
        want, want2 = host.reproject_motion(*MO.args(c), history_variance=c["hvar"], **DEFAULTS)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got2), bits(want2)), name
        got = host.reproject_deform(*MO.args(c), hit, verts, verts.copy(), **DEFAULTS)
        assert np.array_equal(bits(got), bits(host.reproject_motion(*MO.args(c), **DEFAULTS))), name
        if name == "translated":
            assert (want[..., 3] > 0).mean() > 0.3


# ---- 3. a rigid motion expressed as a deformation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0.031, 0.0, 0.0), (-0.052, 0.027, 0.0), (0.06, -0.06, 0.0)])
def test_translation_as_deformation_agrees_with_translation_as_motion(host, shift):
    """One quad mesh that faces the camera and fills a 64 x 48 frame (one instance, one normal, one leaf type), a history whose rgb
    is affine in the pixel coordinates with a constant count, and a translation of at most 2 pixels applied (a) to the vertices,
    reprojected by the deform path, and (b) to the instance matrix, reprojected by polaris_host_reproject_motion.  The two source
    points differ by a few ulp, about 1e-6 relative: below 1e-4 pixel here; the history is linear, so h differs by that times the
    gradient -- the bound, 1e-4 of the history's range, keeps two orders of margin.  Both find history on at least 90 % of the
    pixels (a 2-pixel shift loses at most 2 of 64 columns)."""
    from polaris_amd import scenes as S

    W, H = 64, 48
    e, f = TO.pinhole((0, 0, 0), aspect=W / H)
    z = -4.0
    half_h = abs(z) * np.tan(np.radians(45.0) / 2)                     # the frame at the quad's depth; one pixel is 2 half_h / H wide
    pixel = 2 * half_h / H
    assert max(abs(shift[0]), abs(shift[1])) <= 2 * pixel
    old = VO.quad_tris(-3.0, 3.0, -2.5, 2.5, z)
    tri_inst, tri_leaf = np.zeros(2, int), np.full(2, T.BXDF_DIFFUSE)
    new = old.copy()
    new[:, :3] = (old[:, :3].astype(np.float64) + np.asarray(shift)).astype(F)
    eye4, moved = np.eye(4), S.translation(shift)
    pg, pa, pi, _ = VO.cast(e, f, W, H, old, tri_inst, tri_leaf, [eye4])
    assert G.filtered_mask(pa).all()
    gy, gx = np.mgrid[0:H, 0:W]
    hist = np.zeros((H, W, 4), F)
    hist[..., 0], hist[..., 1], hist[..., 2] = 0.5 + 0.01 * gx, 2.0 - 0.02 * gy, 1.0 + 0.005 * gx + 0.01 * gy
    hist[..., 3] = 16
    span = float(hist[..., :3].max() - hist[..., :3].min())
    # (a) the vertices moved, the matrix did not; (b) the matrix moved, the vertices did not
    ga, aa, ia, hita = VO.cast(e, f, W, H, new, tri_inst, tri_leaf, [eye4])
    gb, ab, ib, _ = VO.cast(e, f, W, H, old, tri_inst, tri_leaf, [moved])
    ident, inv_moved = MO.inv16(eye4)[None], MO.inv16(moved)[None]
    a = host.reproject_deform(hist, pg, pa, pi, e, f, ga, aa, ia, e, f, ident, ident, hita, new, old, **DEFAULTS)
    b = host.reproject_motion(hist, pg, pa, pi, e, f, gb, ab, ib, e, f, ident, inv_moved, **DEFAULTS)
    both = (a[..., 3] > 0) & (b[..., 3] > 0)
    diff = np.abs(a[both, :3] - b[both, :3]).max()
    print(f"shift {shift}: both have history on {100 * both.mean():.1f} % of the pixels, (b) alone {100 * (b[..., 3] > 0).mean():.1f} %, "
          f"largest |h_a - h_b| = {diff:.2e} = {diff / span:.2e} of the history's range")
    assert (b[..., 3] > 0).mean() >= 0.9
    assert both.mean() >= 0.9
    assert diff <= 1e-4 * span
    np.testing.assert_allclose(a[both, 3], b[both, 3], atol=1e-3)
    # and it is the history a pixel `shift` away: the deform path does not return the history at the same pixel
    same_pixel = np.abs(a[both, :3] - hist[both, :3]).max()
    assert same_pixel > 10 * 1e-4 * span


# ---- 4. the snapshot rule ---------------------------------------------------------------------------------------------------------
CAPTURE = "0x200b"            # TEMPORAL, GUIDE, ALBEDO and INSTANCE are swapped with their history twins
EXPECTED = f"""
sync deform sync | sync | reads history 0 | deform kernel 0 | HIT plane 1
sync deform sync | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
sync deform sync | sync | reads history 1 | deform kernel 1 | HIT plane 1
sync camera deform | sync | reads history 0 | deform kernel 0 | HIT plane 1
sync camera deform | camera | planes {CAPTURE} | snapshot 0 | history 1 | has_snapshot 0
sync camera deform | deform | planes 0x0 | snapshot 1 | history 1 | has_snapshot 1
sync camera deform | sync | reads history 1 | deform kernel 1 | HIT plane 1
sync deform deform | sync | reads history 0 | deform kernel 0 | HIT plane 1
sync deform deform | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
sync deform deform | deform | planes 0x0 | snapshot 0 | history 1 | has_snapshot 1
sync deform deform | sync | reads history 1 | deform kernel 1 | HIT plane 1
sync deform sync deform | sync | reads history 0 | deform kernel 0 | HIT plane 1
sync deform sync deform | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
sync deform sync deform | sync | reads history 1 | deform kernel 1 | HIT plane 1
sync deform sync deform | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
sync deform sync deform | sync | reads history 1 | deform kernel 1 | HIT plane 1
deform without history | deform | planes 0x0 | snapshot 0 | history 0 | has_snapshot 0
deform without history | sync | reads history 0 | deform kernel 0 | HIT plane 1
sync deform material | sync | reads history 0 | deform kernel 0 | HIT plane 1
sync deform material | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
sync deform material | material | planes 0x0 | snapshot 0 | history 0 | has_snapshot 0
sync deform material | sync | reads history 0 | deform kernel 0 | HIT plane 1
option toggled | sync | reads history 0 | deform kernel 0 | HIT plane 1
option toggled | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
option toggled | option off | planes 0x10000 | snapshot 0 | history 0 | has_snapshot 0
option toggled | sync | reads history 0 | deform kernel 0 | HIT plane 0
option toggled | deform | planes 0x0 | snapshot 0 | history 0 | has_snapshot 0
option toggled | option on | planes 0x0 | snapshot 0 | history 0 | has_snapshot 0
option toggled | sync | reads history 0 | deform kernel 0 | HIT plane 1
option toggled | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
option toggled | sync | reads history 1 | deform kernel 1 | HIT plane 1
resize | sync | reads history 0 | deform kernel 0 | HIT plane 1
resize | deform | planes {CAPTURE} | snapshot 1 | history 1 | has_snapshot 1
resize | resize | planes 0xffff | snapshot 0 | history 0 | has_snapshot 0
resize | sync | reads history 0 | deform kernel 0 | HIT plane 1
option off | sync | reads history 0 | deform kernel 0 | HIT plane 0
option off | deform | planes 0x0 | snapshot 0 | history 0 | has_snapshot 0
option off | sync | reads history 0 | deform kernel 0 | HIT plane 0
"""


def test_snapshot_rule_of_the_sync_state():
    """tests/tools/vertex_motion_state_check.cpp drives SyncState as the library does and prints what the owner is told; the table
    above is written from the rule's statement: a snapshot is taken just before an update overwrites vertices a
    history was seen with -- also when the capture happened at an earlier camera move -- and never twice for one history; a dropped
    history has none.  Built with the address and undefined-behaviour sanitizers, as a host program."""
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    src = os.path.join(ROOT, "tests", "tools", "vertex_motion_state_check.cpp")
    exe = os.path.join(build, "vertex_motion_state_check")
    deps = [src, os.path.join(ROOT, "polaris_amd", "csrc", "frame_sync.h"), os.path.join(ROOT, "include", "polaris_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip().splitlines() == EXPECTED.strip().splitlines()


# ---- 5. quality -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quality_small(host, oracle, seed):
    """The 64^2 variant of scripts/vertex_motion_quality.py (profiles/vertex_motion_quality.txt has the 128^2 figures): on every seed
    the feature beats the dropped history over all filtered pixels, and the history kept with the rigid arithmetic over the
    deformed block's pixels.  Measured at 64^2 (a/b all, a/c block): seed 0 0.135, 0.675; seed 1 0.161, 0.762; seed 2 0.128, 0.793."""
    res = VO.quality_run(host, oracle, 1, N=64, ref_spp=1024, report=(1,), seed=seed)[1]
    print(f"seed {seed}: " + "  ".join(f"{s} {' '.join(f'{n} {v:.4f}' for n, v in res[s].items())}" for s in "abc") +
          f"  a/b all {res['a']['all'] / res['b']['all']:.3f}  a/c block {res['a']['block'] / res['c']['block']:.3f}  reused {res['reused']:.3f} pixels {res['pixels']}")
    assert res["pixels"]["block"] > 100 and res["reused"] > 0.5
    assert res["a"]["all"] < res["b"]["all"]
    assert res["a"]["block"] < res["c"]["block"]


# ---- 6. the example driver ----------------------------------------------------------------------------------------------------------
def test_render_ripple_argument():
    from polaris_amd import render

    assert render.parse_ripple("0.02:0.5") == (0.02, 0.5)
    for bad in ("", "0.02", "0.02:0", "a:b", "0.1:-2"):
        with pytest.raises(ValueError):
            render.parse_ripple(bad)
    with pytest.raises(SystemExit):
        render.main(["scene.obj", "--ripple", "0.02:0.5"])                 # (needs --frames)
