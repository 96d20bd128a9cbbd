"""CPU tests of the orthographic and equirectangular cameras (include/polaris_hip.h: polaris_hip_set_projection):
the struct as the C compiler lays it out, the geometry of the restated rays (tests/projection_oracle.py), the round trip of every
pixel's centre ray through the header's own inverse (polaris_amd/csrc/temporal.h tp_project, called through the host library), and the
identity reprojection: with the history camera equal to the current one every filtered pixel takes history.

Round trip, measured here on the 64 x 32 frame (pixels; the bar is 2^-10 = 9.8e-4), t = 0.5, 7 and 1000 x the scene's extent:
  equirectangular   2.5e-5 in x (at t = 0.5 x), 1.9e-6 in y, on the frustum's basis and on the turned one;
  orthographic      1.9e-6 on the frustum's basis; on the turned basis 5.7e-6, 5.7e-6 and 9.9e-5 in x (4.0e-5 in y).  Its window is
                    round_trip_window's, 27.5 x 13.7 world units, sized from the rounding that the float32 point and basis the test
                    hands over carry by themselves: a parallel projection does not shrink a sideways offset with distance.  With a
                    window as high as the scene's extent (a pixel of 0.0315) the case turned, t = 1000 x measures 1.36e-3, ABOVE the bar.
dist is within 1.1e-6 relative of t everywhere (the bar is 1e-5).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import projection_oracle as PO
from conftest import ROOT, bits
from polaris_amd import ctypes_api as T

F = np.float32
KINDS = [PO.ORTHOGRAPHIC, PO.EQUIRECTANGULAR]
SEEDS = [7, 0x9E3779B9, 0xFFFFFFF0, 123456789]      # (0xFFFFFFF0: gx + seed wraps)


def cornell(W, H):
    from polaris_amd import scenes

    return scenes.SCENES["cornell"](W / H)


# ---- the ABI (beside test_abi.py)
def test_projection_params_layout_as_the_c_compiler_sees_it(tmp_path):
    fields = ["struct_size", "kind", "axis", "right", "up", "half_width", "half_height", "lon_range", "lat_range"]
    src = tmp_path / "projection.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "polaris_hip.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(PolarisProjectionParams), '
                   + ", ".join("offsetof(PolarisProjectionParams, %s)" % f for f in fields)
                   + "); printf(\"%d %d %d\\n\", POLARIS_PROJECTION_PERSPECTIVE, POLARIS_PROJECTION_ORTHOGRAPHIC, POLARIS_PROJECTION_EQUIRECTANGULAR); return 0; }\n")
    exe = tmp_path / "projection"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [60, 0, 4, 8, 20, 32, 44, 48, 52, 56, 0, 1, 2]
    P = T.ProjectionParams
    assert [C.sizeof(P)] + [getattr(P, f).offset for f in fields] == got[:10]
    assert P().struct_size == 60 and P().kind == 0
    assert (T.PROJECTION_PERSPECTIVE, T.PROJECTION_ORTHOGRAPHIC, T.PROJECTION_EQUIRECTANGULAR) == (0, 1, 2)
    assert "polaris_hip_set_projection" in T.C_ABI_SYMBOLS


def test_set_projection_refuses_a_null_handle(built):
    lib = T.load_library()
    p = T.projection_params()
    assert lib.polaris_hip_set_projection(None, C.byref(p)) == 2       # POLARIS_E_BAD_ARGUMENT
    assert lib.polaris_hip_set_projection(None, None) == 2


# ---- the restated rays
@pytest.mark.parametrize("turned", [False, True])
def test_orthographic_rays_are_the_axis_and_start_inside_the_window(oracle, turned):
    W, H = 16, 9
    sc = cornell(W, H)
    proj = PO.scene_projection(sc, PO.ORTHOGRAPHIC, turned)
    eye = np.asarray(sc.eye, np.float64)
    ax, rt, up = (x.astype(np.float64) for x in (proj.axis, proj.right, proj.up))
    for seed in SEEDS:
        rays = PO.projection_rays(oracle, sc.eye, proj, W, H, 0, H, seed)
        assert np.array_equal(bits(rays[:, 4:7]), np.broadcast_to(bits(proj.axis), (W * H, 3)))     # the axis, bit for bit
        assert np.array_equal(bits(rays[:, 3]), np.full(W * H, bits(PO.FLT_MAX))) and np.array_equal(rays[:, 7], np.arange(W * H, dtype=F))
        q = rays[:, 0:3].astype(np.float64) - eye
        assert np.abs(q @ ax).max() <= 1e-6 * PO.scene_extent(sc)                                   # in the plane through the eye
        a, b = q @ rt, q @ up
        # inside the window -- of the samples: the tent filter's offset lies in [-0.5, 1.5), so an edge pixel's sample reaches half a pixel
        # (1 / W of the half width) beyond the window of the pixel centres, as the perspective camera's does beyond its frustum
        assert np.abs(a).max() <= float(proj.half_width) * (1 + 1 / W + 1e-6) and np.abs(b).max() <= float(proj.half_height) * (1 + 1 / H + 1e-6)
        # ... and pixel (gx, gy) stays within a pixel of its cell's centre
        gx, gy = np.arange(W * H) % W, np.arange(W * H) // W
        assert np.all(np.abs(a / float(proj.half_width) - (2 * (gx + 0.5) / W - 1)) <= 2 / W + 1e-6)
        assert np.all(np.abs(b / float(proj.half_height) - (1 - 2 * (gy + 0.5) / H)) <= 2 / H + 1e-6)
        assert a[0] < 0 < b[0]                                                                      # pixel (0, 0): toward -right, +up
    centre = PO.centre_rays(oracle, sc.eye, proj, W, H)
    q = centre[:, 0:3].astype(np.float64) - eye
    assert np.abs(q @ rt).max() < float(proj.half_width) and np.abs(q @ up).max() < float(proj.half_height)     # the centre rays: strictly inside
    assert np.allclose(q @ rt / float(proj.half_width), 2 * (np.arange(W * H) % W + 0.5) / W - 1, atol=1e-6)
    assert np.allclose(q @ up / float(proj.half_height), 1 - 2 * (np.arange(W * H) // W + 0.5) / H, atol=1e-6)


@pytest.mark.parametrize("turned", [False, True])
def test_equirectangular_rays_are_unit_vectors_around_the_basis(oracle, turned):
    W, H = 64, 32
    sc = cornell(W, H)
    proj = PO.scene_projection(sc, PO.EQUIRECTANGULAR, turned)
    ax, rt, up = (x.astype(np.float64) for x in (proj.axis, proj.right, proj.up))
    for seed in SEEDS:
        rays = PO.projection_rays(oracle, sc.eye, proj, W, H, 0, H, seed)
        d = rays[:, 4:7].astype(np.float64)
        assert np.abs((d * d).sum(axis=1) - 1).max() <= 4 * 2.0 ** -23
        assert np.array_equal(bits(rays[:, 0:3]), np.broadcast_to(bits(np.asarray(sc.eye, F)), (W * H, 3)))
    d = PO.centre_rays(oracle, sc.eye, proj, W, H)[:, 4:7].astype(np.float64).reshape(H, W, 3)
    pixel_lon, pixel_lat = 2 * np.pi / W, np.pi / H
    assert np.arccos(np.clip(d[H // 2, W // 2] @ ax, -1, 1)) <= max(pixel_lon, pixel_lat)          # the pixel nearest the centre looks along the axis
    assert np.all(np.arccos(np.clip(d[0] @ up, -1, 1)) <= pixel_lat)                              # row 0 points to +up
    assert np.all(np.arccos(np.clip(d[H - 1] @ -up, -1, 1)) <= pixel_lat)
    assert (d[H // 2, W // 2 + W // 4] @ rt) > 0.99                                               # a quarter of the frame to the right: +right


def test_the_host_librarys_guide_rays_are_the_restatements(built, oracle):
    """The header's tp_guide_ray (what k_gbuffer_proj casts) against numpy, bit for bit: the round trip below starts from rays both agree on."""
    from polaris_amd import host_api

    W, H = 64, 32
    sc = cornell(W, H)
    for kind in KINDS:
        for turned in (False, True):
            proj = PO.scene_projection(sc, kind, turned)
            rays = PO.centre_rays(oracle, sc.eye, proj, W, H)
            o, d = host_api.projection_rays(proj.params(), sc.eye, W, H)
            assert np.array_equal(bits(o), bits(rays[:, 0:3])) and np.array_equal(bits(d), bits(rays[:, 4:7])), (kind, turned)


# ---- the round trip
ROUND_TRIP_SCALES = [0.5, 7.0, 1000.0]


def round_trip_window(extent, W, H, bar=2.0 ** -10):
    """(half_width, half_height) of the orthographic window of the round trip, from the precision of float32 alone.

    The test hands tp_project a float32 point and a float32 basis, and both carry an error of their own before tp_project computes
    anything.  At the largest t = 1000 x the extent, in world units across the axis:
      the point     each coordinate is the ray's point rounded once, off by at most half a spacing of float32 at that distance, h;
                    against a unit vector that is at most sqrt(3) h;
      the basis     axis, right and up are unit vectors rounded to float32, each entry off by at most 2^-25, so a pair's dot product
                    is off from 0 by at most 2 sqrt(3) 2^-25, and a point t along the axis appears that much x t to the side.
    A parallel projection does not shrink such an offset with distance (the panorama's angles do), so in pixels it is the offset over
    the pixel's width.  The window is the one whose pixel makes that bound half the bar, which leaves the other half to tp_project;
    square pixels.  With the scene's extent as the window's height (a pixel of 0.0315) the same inputs measure 1.36e-3 pixel at
    t = 1000 x, above the bar, and 1.5e-5 at t = 7 x: DESIGN.md 10n records it."""
    t_max = max(ROUND_TRIP_SCALES) * extent
    h = float(np.spacing(F(2.0 * t_max))) / 2             # (the points lie within twice t_max of the origin)
    offset = np.sqrt(3.0) * h + 2 * np.sqrt(3.0) * 2.0 ** -25 * t_max
    pixel = offset / (bar / 2)
    return 0.5 * W * pixel, 0.5 * H * pixel


@pytest.mark.parametrize("scale", ROUND_TRIP_SCALES)
@pytest.mark.parametrize("turned", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_every_pixel_comes_back_from_its_point_on_the_centre_ray(built, oracle, kind, turned, scale):
    from polaris_amd import host_api

    W, H = 64, 32
    sc = cornell(W, H)
    proj = PO.scene_projection(sc, kind, turned)
    if kind == PO.ORTHOGRAPHIC:
        proj.half_width, proj.half_height = (F(x) for x in round_trip_window(PO.scene_extent(sc), W, H))
    rays = PO.centre_rays(oracle, sc.eye, proj, W, H)
    t = F(scale * PO.scene_extent(sc))
    points = (rays[:, 0:3].astype(np.float64) + rays[:, 4:7].astype(np.float64) * float(t)).astype(F)      # the ray's point, rounded once
    uvd, ok = host_api.projection_project(proj.params(), sc.eye, points)
    assert ok.all()
    x, y = uvd[:, 0].astype(np.float64) * W - 0.5, uvd[:, 1].astype(np.float64) * H - 0.5
    gx, gy = np.arange(W * H) % W, np.arange(W * H) // W
    dx, dy, dd = np.abs(x - gx).max(), np.abs(y - gy).max(), np.abs(uvd[:, 2].astype(np.float64) / float(t) - 1).max()
    print(f"round trip kind {kind} turned {turned} t {scale} x extent: dx {dx:.3g} px  dy {dy:.3g} px  dist {dd:.3g} relative")
    assert dd <= 1e-5
    assert dx <= 2.0 ** -10 and dy <= 2.0 ** -10


# ---- the identity reprojection
def identity_scenes(W, H):
    from polaris_amd import scenes

    return {"cornell": cornell(W, H), "moving-instances": scenes.moving_instances(0, W / H)}


# the orthographic window, the whole panorama (in which a scene seen from outside fills a few dozen pixels) and a third of it each way
IDENTITY_CAMERAS = {"orthographic": (PO.ORTHOGRAPHIC, {}), "panorama": (PO.EQUIRECTANGULAR, {}),
                    "partial-panorama": (PO.EQUIRECTANGULAR, dict(lon_range=2 * np.pi / 3, lat_range=np.pi / 3))}


@pytest.mark.parametrize("name", ["cornell", "moving-instances"])
@pytest.mark.parametrize("camera", list(IDENTITY_CAMERAS))
def test_with_the_history_camera_equal_to_the_current_one_every_filtered_pixel_takes_history(built, oracle, camera, name):
    import gbuffer_oracle as GO
    from polaris_amd import host_api

    W, H = 40, 20
    sc = identity_scenes(W, H)[name]
    kind, ranges = IDENTITY_CAMERAS[camera]
    proj = PO.scene_projection(sc, kind, True, **ranges)
    guide, albedo = PO.gbuffer(oracle, sc, PO.centre_rays(oracle, sc.eye, proj, W, H), W, H)
    filtered = GO.filtered_mask(albedo)                     # a hit that is not an emitter (denoise.h dn_filtered)
    assert filtered.sum() >= (W * H // 8 if camera != "panorama" else 12), "the camera sees too little of the scene"
    history = np.ones((H, W, 4), F)
    prior = host_api.reproject_projection(history, guide, albedo, sc.eye, guide, albedo, sc.eye, proj.params())
    took = prior[..., 3] > 0
    assert np.array_equal(took, filtered), (int((filtered & ~took).sum()), int((took & ~filtered).sum()))
    assert np.array_equal(bits(prior[filtered]), np.broadcast_to(bits(np.ones(4, F)), (int(filtered.sum()), 4)))    # ones in, ones out
