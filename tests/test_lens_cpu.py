"""The thin-lens generator's statement (tests/lens_oracle.py) checked on its own, without a GPU: the lens points
fill the unit disk uniformly, every ray passes through its pinhole ray's point on the plane of focus, and the rays of one pixel
converge at the focus distance and spread by the aperture away from it.  The GPU tests (test_gpu_lens.py) then hold the kernel to
this statement bit for bit.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_oracle as LO
from conftest import ROOT

W, H, BY, BH = 24, 10, 3, 6      # rows [3, 9): N = 144, one partly filled chunk
SEEDS = [(0x9E3779B9 * (k + 1)) & 0xFFFFFFFF for k in range(16)]
RADIUS, FOCUS = 0.05, 1.9        # 0.05 x the Cornell box's extent (~1); the plane of focus lies inside the box


@pytest.fixture(scope="module")
def cornell():
    from polaris_amd import scenes

    return scenes.SCENES["cornell"](W / H)


@pytest.fixture(scope="module")
def rays(oracle, cornell):
    """Per seed: the restated rays of the block with their details.  Computed once, shared unchanged."""
    lens = LO.Lens.from_frustum(cornell.frustum, RADIUS, FOCUS)
    out = []
    for seed in SEEDS:
        r, det = LO.lens_rays(oracle, cornell, lens, W, H, BY, BH, seed, details=True)
        r.setflags(write=False)
        out.append((r, det))
    return lens, out


def test_lens_points_lie_in_the_unit_disk(rays):
    _, per_seed = rays
    for _, det in per_seed:
        lx, ly = det["lx"].astype(np.float64), det["ly"].astype(np.float64)
        assert (lx * lx + ly * ly <= 1 + 2.0 ** -22).all()


def test_lens_points_are_uniform_over_the_disk(oracle):
    """4 096 draws: the disk of radius 0.5 holds a quarter of the area, so its share is binomial with sigma = sqrt(0.25 * 0.75 / 4096)
    = 0.0068; four of them are 0.027 (0.03).  A coordinate of a uniform disk point has variance 1/4: the mean's sigma is 0.0078."""
    draws = []
    seed = 1
    while sum(len(d) for d in draws) < 4096:
        draws.append(LO.camera_draws(oracle, W, BH, (0x85EBCA6B * seed) & 0xFFFFFFFF)[1])
        seed += 1
    s1 = np.concatenate(draws)[:4096]
    lx, ly = LO.disk_points(oracle, s1)
    r2 = lx.astype(np.float64) ** 2 + ly.astype(np.float64) ** 2
    share = float((r2 <= 0.25).mean())
    print("share within radius 0.5:", share, "mean:", float(lx.mean()), float(ly.mean()))
    assert abs(share - 0.25) <= 0.03
    assert np.hypot(float(lx.mean(dtype=np.float64)), float(ly.mean(dtype=np.float64))) <= 0.05


def test_every_ray_passes_through_its_focus_point(rays, cornell):
    """The focus point is P = eye + d ft with the float32 d and ft taken exactly.  The exact line from the exact lens point E = eye + L
    through P has direction P - E = d ft - L.  What the restatement rounds, with e = 2^-24 and |q| <= ft + |u| + |v|:
      q_k = fl(fl(d_k ft) - L_k): at most e (|d_k| ft + |q_k|) per component, at most 2 e sqrt(3) (ft + |u| + |v|) as a vector;
      L_k = fl(fl(lx u_k) + fl(ly v_k)): moves E and q together (the line through P turns about P: no miss at P beyond second order);
      origin_k = fl(eye_k + L_k): at most e (|eye_k| + |L_k|), as a vector e sqrt(3) (max|eye| + |u| + |v|);
      direction_k = fl(q_k inv2): inv2's own error is common to the three components and turns nothing; the product's rounding
      turns the direction by at most e sqrt(3), which over the distance |q| to P is e sqrt(3) (ft + |u| + |v|).
    Sum: below e sqrt(3) (3 ft + max|eye| + 4 (|u| + |v|)) < 7 * 2^-24 * (max|eye| + ft + |u| + |v|), i.e. 3.5 * 2^-23 of the
    scale; the bound is 16 * 2^-23 of it."""
    lens, per_seed = rays
    eye = np.asarray(cornell.eye, np.float64)
    nu, nv = np.linalg.norm(lens.u.astype(np.float64)), np.linalg.norm(lens.v.astype(np.float64))
    worst = 0.0
    for r, det in per_seed:
        assert det["on"].all()      # every Cornell camera ray looks along the axis
        ft = det["ft"].astype(np.float64)
        P = eye[None, :] + det["d"].astype(np.float64) * ft[:, None]
        o, d = r[:, 0:3].astype(np.float64), r[:, 4:7].astype(np.float64)
        w = P - o
        miss = np.linalg.norm(w - d * (np.sum(w * d, axis=1) / np.sum(d * d, axis=1))[:, None], axis=1)
        bound = 16 * 2.0 ** -23 * (np.abs(eye).max() + ft + nu + nv)
        worst = max(worst, float((miss / bound).max()))
        assert (miss <= bound).all()
        assert (np.abs(np.linalg.norm(d, axis=1) - 1) <= 4 * 2.0 ** -24).all()      # unit directions
        assert (r[:, 3] == LO.FLT_MAX).all()
    print("largest miss / bound:", worst)


FINE_W, FINE_H, FINE_BY, FINE_BH = 480, 200, 99, 3     # a frame whose pixels are small beside the aperture
PIXEL = (241, 1)    # of that block's 480 x 3 pixels: one near the frame's centre
SPREAD_SEEDS = [(0xC2B2AE35 * (k + 1)) & 0xFFFFFFFF for k in range(32)]


def _hits_on_plane(oracle, sc, lens, z):
    """Where the 32 rays of PIXEL meet the plane perpendicular to the axis at distance z from the eye (the scene's one quad), float64."""
    eye, ax = np.asarray(sc.eye, np.float64), lens.axis.astype(np.float64)
    pts = []
    for seed in SPREAD_SEEDS:
        r = LO.lens_rays(oracle, sc, lens, FINE_W, FINE_H, FINE_BY, FINE_BH, seed, paths=[PIXEL[1] * FINE_W + PIXEL[0]])[0].astype(np.float64)
        o, d = r[0:3], r[4:7]
        t = (z - np.dot(o - eye, ax)) / np.dot(d, ax)
        pts.append(o + t * d)
    pts = np.array(pts)
    return np.linalg.norm(pts[:, None, :] - pts[None, :, :], axis=-1)


def test_rays_of_a_pixel_converge_at_the_focus_distance_and_spread_away_from_it(oracle, cornell):
    z = 2.0
    fr = np.asarray(cornell.frustum, np.float64).reshape(4, 4)[:, :3]
    axis = LO.Lens.from_frustum(cornell.frustum, RADIUS, z).axis.astype(np.float64)
    scale = z / np.dot(fr[0], axis)                       # the corner rays reach the plane at this multiple
    pw, ph = np.linalg.norm(fr[1] - fr[0]) * scale / FINE_W, np.linalg.norm(fr[0] - fr[2]) * scale / FINE_H
    footprint = np.hypot(2 * pw, 2 * ph)                 # the tent filter spans 2 x 2 pixels: its diagonal
    focused = _hits_on_plane(oracle, cornell, LO.Lens.from_frustum(cornell.frustum, RADIUS, z), z)
    defocused = _hits_on_plane(oracle, cornell, LO.Lens.from_frustum(cornell.frustum, RADIUS, z / 2), z)
    print("focused:", float(focused.max()), "footprint:", footprint, "defocused:", float(defocused.max()), "radius:", RADIUS)
    assert focused.max() <= footprint
    assert defocused.max() > 0.5 * RADIUS
    assert footprint < 0.5 * RADIUS                     # (the two statements tell the cases apart)


def test_lens_from_frustum_on_the_cornell_camera(cornell):
    from polaris_amd import ctypes_api as T

    axis, u, v = T.lens_from_frustum(cornell.frustum, RADIUS)
    assert axis.dtype == u.dtype == v.dtype == np.float32
    a, u, v = (x.astype(np.float64) for x in (axis, u, v))
    assert abs(np.linalg.norm(a) - 1) <= 1e-6
    assert abs(np.dot(a, u)) <= 1e-6 and abs(np.dot(a, v)) <= 1e-6
    assert abs(np.linalg.norm(u) - RADIUS) <= 1e-6 and abs(np.linalg.norm(v) - RADIUS) <= 1e-6
    assert a[2] > 0.999 and u[0] != 0 and v[1] > 0      # looks down +z; u runs along the image's x, v up


def test_focus_pixel_takes_the_distance_along_the_axis_from_the_guide_plane(cornell):
    """render.py --focus-pixel: t * dot(centre direction, axis) of the GUIDE plane's first hit; a miss is an error."""
    from polaris_amd import render

    guide = np.zeros((H, W, 4), np.float32)
    guide[..., 3] = 2.5
    guide[0, 0, 3] = LO.FLT_MAX
    fr = np.asarray(cornell.frustum, np.float64).reshape(4, 4)[:, :3]
    on_axis = render.focus_of_pixel(guide, cornell.frustum, W // 2, H // 2)
    corner = render.focus_of_pixel(guide, cornell.frustum, W - 1, H - 1)
    # the corner rays reach the near plane (axis distance 1) after |corner| along themselves: cos = 1 / |corner|, a little more for a pixel centre inside the frame
    assert 2.5 / np.linalg.norm(fr[3]) < corner < on_axis < 2.5 and on_axis > 2.5 * 0.99
    with pytest.raises(ValueError, match="sees nothing"):
        render.focus_of_pixel(guide, cornell.frustum, 0, 0)
    with pytest.raises(ValueError, match="outside"):
        render.focus_of_pixel(guide, cornell.frustum, W, 0)


# ---- the ABI (beside test_abi.py)

def test_lens_params_layout_as_the_c_compiler_sees_it(tmp_path):
    from polaris_amd import ctypes_api as T

    src = tmp_path / "lens.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "polaris_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(PolarisLensParams), offsetof(PolarisLensParams, struct_size), offsetof(PolarisLensParams, focus_distance), '
                   'offsetof(PolarisLensParams, axis), offsetof(PolarisLensParams, u), offsetof(PolarisLensParams, v)); return 0; }\n')
    exe = tmp_path / "lens"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [44, 0, 4, 8, 20, 32]
    P = T.LensParams
    assert [C.sizeof(P), P.struct_size.offset, P.focus_distance.offset, P.axis.offset, P.u.offset, P.v.offset] == got
    assert P().struct_size == 44
    assert "polaris_hip_set_lens" in T.C_ABI_SYMBOLS


def test_set_lens_refuses_a_null_handle(built):
    from polaris_amd import ctypes_api as T

    lib = T.load_library()
    p = T.lens_params()
    assert lib.polaris_hip_set_lens(None, C.byref(p)) == 2       # POLARIS_E_BAD_ARGUMENT
    assert lib.polaris_hip_set_lens(None, None) == 2
