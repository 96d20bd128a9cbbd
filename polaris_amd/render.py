"""Render a Wavefront scene to a PNG on the MI355X backend -- an example driver, not a CLI clone.

    python -m polaris_amd.render scene.obj --width 512 --height 512 --spp 128 --out frame.png

Flags and defaults are those of `polaris render` (cmd/render.go:17-60, cmd/main.go): the scene goes
through the C++ reader/compiler (polaris_amd/host), the frame through the C++ DefaultRenderer
(renderer/default.go's loop) over HipTracers, one per requested device.  RR is disabled the way
the reference does it (rr-bounces 0 or >= num-bounces -> num-bounces + 1).

--denoise N filters the synced frame with N iterations of the edge-avoiding a-trous filter (polaris_hip_set_denoise, the
other settings at their defaults); --aov-dir DIR also writes the first-hit guide planes as normals.png / depth.png (the byte
formulas of the reference's debug kernels, tracer/opencl/CL/kernels/debug.cl) and albedo.png.

--guide-specular N lets the guide ray of that G-buffer follow up to N mirror and glass interactions (the tracer option "guide_specular",
DESIGN.md 10i; 0..8, 0 = the first hit): what --denoise, --temporal and --aov-dir then see inside a mirror is the reflected surface.

--frames N --move DIR:OFFSET renders N frames, each one render(accumulated=0) after a camera move (scene.Camera.Move, camera.go:76-97,
DIR one of left, right, up, down, forward, backward), written as <out stem>_000.png, _001.png, ...: what the interactive renderer
does while the user moves.  --temporal M reuses the last view's mean across the moves with max_history M (polaris_hip_set_temporal,
the thresholds at their defaults).

--variance SIGMA guides the filter by each pixel's variance (polaris_hip_set_variance with sigma_variance SIGMA, min_samples at its
default, the option moments on every tracer; 0 = off); with --aov-dir the VARIANCE plane (M1 | M2 | n_eff | v) is also written as
variance.npy.

--frames N --recolour NODE:r,g,b[:step] renders N frames with an edit of a material per frame instead of a camera move: frame k gives
material node NODE the colour (r, g, b) + k * step * (1, 1, 1) through polaris_hip_update_materials -- the node
table in place, no upload_scene -- then render(accumulated=0).

--frames N --ripple AMPLITUDE:WAVELENGTH renders N frames with a deformation of the scene's meshes per frame instead of a camera move:
frame k displaces every vertex along y by AMPLITUDE * sin(2 pi (x + z) / WAVELENGTH + k) (mesh space) through
polaris_hip_update_vertices -- the arrays in place, no upload_scene -- then render(accumulated=0).  With --temporal
the options "object_motion" and "vertex_motion" are on, so the history is carried across every deformation.

--aperture R --focus D renders through a thin lens of radius R focused at distance D along the view axis (polaris_hip_set_lens,
DESIGN.md 10h; it stays on the camera through --frames moves).  --focus-pixel x,y takes D from the GUIDE plane instead: the first hit
under that pixel's centre, t * dot(centre direction, axis); a pixel that sees nothing is an error.

--projection orthographic --ortho-height F renders through a window F scene units high with parallel rays; --projection equirect
renders a latitude-longitude panorama of --lon-range x --lat-range degrees (default 360 x 180) around the eye
(polaris_hip_set_projection; either stays on the camera through --frames moves and excludes --aperture and --shutter).

--frames N --shutter F (0 <= F <= 1, default 0 = an instantaneous exposure) leaves the shutter open for the fraction F of the way to
the next frame (polaris_hip_set_shutter): frame k's camera rays spread in time between its camera and the camera one
more move of F * OFFSET on -- camera motion blur.  A lens stays on both ends, with the same radius and focus distance.

--tonemap {reinhard,reinhard-white,aces,hable} [--white W] [--srgb] [--auto-exposure [--ev-comp X] [--adapt A]] replaces the sync's
tone-map by the display transform (polaris_hip_set_display): the tone operator (white: the radiance reinhard-white and
hable map to 1), the sRGB transfer function instead of pow(1 / 2.2), and the frame's own metered exposure (key 0.18, the window
between the median and the 95th percentile; X stops of compensation; A the fraction of the way to the target per frame) times
--exposure.  With --aov-dir the last frame's exposure and histogram are written as exposure.json.  A flag that would be ignored is an
error: --white without reinhard-white or hable, --ev-comp or --adapt without --auto-exposure.

--bloom [INTENSITY] [--bloom-threshold T] [--bloom-levels N] adds bloom to the display transform (polaris_hip_set_bloom): a
bright-pass pyramid of N levels over the displayed values above T, added INTENSITY times before the tone operator (the other fields
are ctypes_api.BLOOM_DEFAULTS).  Bloom is part of the display transform: --bloom without --tonemap, --srgb or --auto-exposure is an
error, and so are --bloom-threshold and --bloom-levels without --bloom."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import ctypes_api as T
from . import host_api


def aov_images(guide: np.ndarray, albedo: np.ndarray) -> dict:
    """RGBA8 images of the GUIDE / ALBEDO planes ((H, W, 4) float32): normals (uchar)((n + 1) * 255 * 0.5) and depth
    (uchar)(255 * (1 - t / (maxDepth + 1))) with maxDepth = max(1, the largest finite t) -- misses (0, 0, 0, 255) -- and albedo
    (uchar)(albedo * 255)."""
    f = np.float32
    t = guide[..., 3]
    hit = t < f(3.0e38)
    max_depth = f(max(1.0, float(t[hit].max()) if hit.any() else 1.0))
    def u8(x):
        return np.clip(x, 0, 255).astype(np.uint8)
    out = {}
    n = np.zeros(guide.shape, np.uint8)
    n[..., :3] = u8((guide[..., :3] + f(1)) * f(255) * f(0.5))
    d = np.zeros(guide.shape, np.uint8)
    d[..., :3] = u8(f(255) * (f(1) - t / (max_depth + f(1))))[..., None]
    n[~hit, :3] = 0
    d[~hit, :3] = 0
    n[..., 3] = d[..., 3] = 255
    a = np.full(albedo.shape, 255, np.uint8)
    a[..., :3] = u8(albedo[..., :3] * f(255))
    out["normals"], out["depth"], out["albedo"] = n, d, a
    return out


def focus_of_pixel(guide: np.ndarray, frustum, x: int, y: int) -> float:
    """The focus distance that puts pixel (x, y)'s first hit in focus: its GUIDE distance t along the pinhole ray through the pixel
    centre, projected onto the view axis.  ValueError outside the frame or where the pixel sees nothing."""
    H, W = guide.shape[:2]
    if not (0 <= x < W and 0 <= y < H):
        raise ValueError(f"--focus-pixel {x},{y}: outside the {W}x{H} frame")
    t = float(guide[y, x, 3])
    if not t < 3.0e38:
        raise ValueError(f"--focus-pixel {x},{y}: the pixel sees nothing to focus on")
    fr = np.asarray(frustum, np.float64).reshape(4, 4)[:, :3]
    tx, ty = (x + 0.5) / W, (y + 0.5) / H
    left, right = fr[0] + (fr[2] - fr[0]) * ty, fr[1] + (fr[3] - fr[1]) * ty
    d = left + (right - left) * tx
    d /= np.sqrt(np.dot(d, d))
    axis = T.lens_from_frustum(frustum, 1.0)[0].astype(np.float64)
    return t * float(np.dot(d, axis))


def parse_move(move: str):
    d, _, off = move.partition(":")
    if d not in host_api.CAMERA_MOVES or not off:
        raise ValueError(f"--move {move!r}: DIR:OFFSET with DIR one of {', '.join(host_api.CAMERA_MOVES)}")
    return d, float(off)


def frame_paths(out: str, n: int) -> list:
    stem, ext = os.path.splitext(out)
    return [f"{stem}_{k:03d}{ext or '.png'}" for k in range(n)]


def move_frames(r, sc, n: int, move: str, aspect: float, shutter: float = 0.0):
    """Frame k: the scene's camera after k + 1 moves (one camera object, as the interactive renderer's), then render(accumulated=0).
    shutter F > 0: the frame's shutter closes at the camera after one more move of F x the offset (set after the camera it belongs to).
    Yields (rows, ms) after each frame."""
    step = parse_move(move)
    for k in range(n):
        eye, fr = host_api.camera_move(sc.camera, [step] * (k + 1), aspect=aspect)
        r.set_camera(eye, fr)
        if shutter:
            r.set_shutter(*host_api.camera_move(sc.camera, [step] * (k + 1) + [(step[0], shutter * step[1])], aspect=aspect))
        yield r.render(0)


def parse_recolour(spec: str, num_nodes: int):
    parts = spec.split(":")
    try:
        node, rgb = int(parts[0]), [float(x) for x in parts[1].split(",")]
        step = float(parts[2]) if len(parts) > 2 else 0.0
    except (ValueError, IndexError):
        node, rgb, step = -1, [], 0.0
    if len(parts) not in (2, 3) or len(rgb) != 3 or not 0 <= node < num_nodes:
        raise ValueError(f"--recolour {spec!r}: NODE:r,g,b[:step] with NODE below {num_nodes}")
    return node, np.array(rgb, np.float32), np.float32(step)


def recolour_frames(r, sc, n: int, spec: str):
    """Frame k: the scene's material nodes with node NODE's k[0..2] = (r, g, b) + k * step, given to every tracer in place
    (Renderer.update_materials: the other arguments are the scene's own), then render(accumulated=0).  Yields (rows, ms)."""
    node, rgb, step = parse_recolour(spec, len(sc.material_nodes))
    nodes = np.ascontiguousarray(sc.material_nodes, dtype=T.MATERIAL_NODE).copy()
    for k in range(n):
        nodes["k"][node][:3] = rgb + np.float32(k) * step
        r.update_materials(nodes, None, int(sc.scene_diffuse_mat_index), None)
        yield r.render(0)


def parse_ripple(spec: str):
    amp, _, wave = spec.partition(":")
    try:
        amp, wave = float(amp), float(wave)
    except ValueError:
        amp, wave = 0.0, 0.0
    if not wave > 0:
        raise ValueError(f"--ripple {spec!r}: AMPLITUDE:WAVELENGTH with WAVELENGTH > 0")
    return amp, wave


def ripple_frames(r, sc, n: int, spec: str, temporal: bool):
    """Frame k: the scene's vertices with y displaced by AMPLITUDE * sin(2 pi (x + z) / WAVELENGTH + k), given to every tracer in place
    (Renderer.update_vertices with the boxes and emissive areas of scenes.refit_vertices), then render(accumulated=0).  The scene is
    uploaded again first, with the option "vertex_update" on -- and, temporal, "object_motion" and "vertex_motion".  Yields (rows, ms)."""
    from . import scenes

    amp, wave = parse_ripple(spec)
    for key in ("vertex_update",) + (("object_motion", "vertex_motion") if temporal else ()):
        r.set_option(key, 1)
    r.upload_scene(sc)
    base = np.ascontiguousarray(sc.vertices, np.float32)
    phase = 2.0 * np.pi * (base[:, 0].astype(np.float64) + base[:, 2].astype(np.float64)) / wave
    for k in range(n):
        v = base.copy()
        v[:, 1] = (base[:, 1].astype(np.float64) + amp * np.sin(phase + k)).astype(np.float32)
        vertices, boxes, _, _, ems = scenes.vertex_update_args(scenes.refit_vertices(sc, v))
        r.update_vertices(vertices, boxes, None, None, ems)
        yield r.render(0)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m polaris_amd.render", description=__doc__.split("\n")[0])
    ap.add_argument("scene", help="scene.obj")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--num-bounces", type=int, default=5)
    ap.add_argument("--rr-bounces", type=int, default=3)
    ap.add_argument("--exposure", type=float, default=1.2)
    ap.add_argument("--out", default="frame.png")
    ap.add_argument("--devices", default="0", help="comma separated HIP device indices (a device may repeat)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--denoise", type=int, default=0, help="a-trous filter iterations at the frame sync (0 = off)")
    ap.add_argument("--variance", type=float, default=0.0, help="sigma_variance of variance-guided denoising (0 = off)")
    ap.add_argument("--aov-dir", default=None, help="write normals.png, depth.png and albedo.png of the first-hit G-buffer here")
    ap.add_argument("--guide-specular", type=int, default=0, help="delta (mirror / glass) links the G-buffer's guide ray follows, 0..8 (0 = first hit)")
    ap.add_argument("--temporal", type=int, default=0, help="max_history of temporal reuse across camera moves (0 = off)")
    ap.add_argument("--frames", type=int, default=0, help="render this many frames, each after a camera move (--move)")
    ap.add_argument("--move", default="right:0.05", help="DIR:OFFSET of every move with --frames (left, right, up, down, forward, backward)")
    ap.add_argument("--recolour", default="", help="NODE:r,g,b[:step]: with --frames, edit material node NODE per frame in place instead of moving the camera")
    ap.add_argument("--ripple", default="", help="AMPLITUDE:WAVELENGTH: with --frames, deform the scene's vertices per frame in place instead of moving the camera")
    ap.add_argument("--aperture", type=float, default=0.0, help="thin-lens radius in scene units (0 = pinhole)")
    ap.add_argument("--focus", type=float, default=0.0, help="with --aperture: distance of the plane of focus along the view axis")
    ap.add_argument("--focus-pixel", default="", help="with --aperture, x,y: focus on what this pixel's centre sees instead of --focus")
    ap.add_argument("--shutter", type=float, default=0.0, help="with --frames (camera moves): the shutter stays open this fraction 0..1 of the way to the next frame (0 = off)")
    ap.add_argument("--projection", choices=sorted(T.PROJECTION_KINDS), default="perspective", help="the camera's projection (orthographic needs --ortho-height)")
    ap.add_argument("--ortho-height", type=float, default=None, help="with --projection orthographic: the height of the window through the eye, scene units")
    ap.add_argument("--lon-range", type=float, default=360.0, help="with --projection equirect: degrees of longitude the frame's width spans")
    ap.add_argument("--lat-range", type=float, default=180.0, help="with --projection equirect: degrees of latitude the frame's height spans")
    ap.add_argument("--tonemap", choices=sorted(T.TONE_OPERATORS), default=None, help="the display transform's tone operator (default: the plain tone-map)")
    ap.add_argument("--white", type=float, default=T.DISPLAY_DEFAULTS["white"], help="with --tonemap reinhard-white / hable: the radiance mapped to 1")
    ap.add_argument("--srgb", action="store_true", help="the sRGB transfer function instead of pow(1 / 2.2)")
    ap.add_argument("--auto-exposure", action="store_true", help="meter every frame and expose it to middle grey")
    ap.add_argument("--ev-comp", type=float, default=0.0, help="with --auto-exposure: exposure compensation in stops")
    ap.add_argument("--adapt", type=float, default=1.0, help="with --auto-exposure: the fraction (0, 1] of the way to the metered exposure per frame")
    ap.add_argument("--bloom", type=float, nargs="?", const=T.BLOOM_DEFAULTS["intensity"], default=None, metavar="INTENSITY",
                    help="with a display flag: add bloom, INTENSITY times the bright-pass pyramid (default %(const)s)")
    ap.add_argument("--bloom-threshold", type=float, default=None, help="with --bloom: the displayed value above which a pixel blooms")
    ap.add_argument("--bloom-levels", type=int, default=None, help="with --bloom: pyramid levels 1..8")
    a = ap.parse_args(argv)
    display = a.tonemap is not None or a.srgb or a.auto_exposure
    if a.bloom is not None and not display:
        ap.error("--bloom needs --tonemap, --srgb or --auto-exposure")
    if (a.bloom_threshold is not None or a.bloom_levels is not None) and a.bloom is None:
        ap.error("--bloom-threshold and --bloom-levels need --bloom")
    if (a.ev_comp or a.adapt != 1.0) and not a.auto_exposure:
        ap.error("--ev-comp and --adapt need --auto-exposure")
    if a.white != T.DISPLAY_DEFAULTS["white"] and a.tonemap not in ("reinhard-white", "hable"):
        ap.error("--white needs --tonemap reinhard-white or hable")
    if not 0.0 <= a.shutter <= 1.0 or (a.shutter and (not a.frames or a.recolour or a.ripple)):
        ap.error("--shutter F needs 0 <= F <= 1, --frames and no --recolour or --ripple")
    if a.ripple and (not a.frames or a.recolour):
        ap.error("--ripple AMPLITUDE:WAVELENGTH needs --frames and no --recolour")
    if a.aperture < 0 or (a.aperture and not a.focus_pixel and not a.focus > 0):
        ap.error("--aperture R needs --focus D > 0 or --focus-pixel x,y")
    if a.projection != "perspective" and (a.aperture or a.shutter):
        ap.error("--projection orthographic / equirect excludes --aperture and --shutter")
    if (a.projection == "orthographic") != (a.ortho_height is not None) or (a.ortho_height is not None and not a.ortho_height > 0):
        ap.error("--projection orthographic needs --ortho-height F > 0, and nothing else takes it")
    if a.projection != "equirect" and (a.lon_range != 360.0 or a.lat_range != 180.0):
        ap.error("--lon-range and --lat-range need --projection equirect")

    rr = a.rr_bounces
    if rr == 0 or rr >= a.num_bounces:
        rr = a.num_bounces + 1
    t0 = time.perf_counter()
    sc = host_api.read_scene(a.scene, aspect=a.width / a.height)
    for w in sc.warnings:
        print("warning:", w, file=sys.stderr)
    t1 = time.perf_counter()
    devs = [int(d) for d in a.devices.split(",")]
    r = host_api.Renderer(sc, devs, width=a.width, height=a.height, spp=a.spp, bounces=a.num_bounces, min_rr=rr,
                          exposure=a.exposure, seed=a.seed)
    try:
        if a.guide_specular:
            r.set_option("guide_specular", a.guide_specular)
        if a.denoise:
            r.set_denoise(iterations=a.denoise)
        if a.temporal:
            r.set_temporal(max_history=a.temporal)
        if a.variance:
            r.set_variance(sigma_variance=a.variance, min_samples=T.VARIANCE_DEFAULTS["min_samples"])
        if display:
            r.set_display(1, tone_operator=a.tonemap or "reinhard", white=a.white, srgb=int(a.srgb), auto_exposure=int(a.auto_exposure),
                          compensation_ev=a.ev_comp, adapt=a.adapt)
        if a.bloom is not None:
            r.set_bloom(1, intensity=a.bloom, threshold=T.BLOOM_DEFAULTS["threshold"] if a.bloom_threshold is None else a.bloom_threshold,
                        levels=T.BLOOM_DEFAULTS["levels"] if a.bloom_levels is None else a.bloom_levels)
        if a.aperture:
            focus = a.focus
            if a.focus_pixel:
                x, _, y = a.focus_pixel.partition(",")
                focus = focus_of_pixel(r.read_aov(T.AOV_GUIDE), sc.frustum, int(x), int(y))
            r.set_lens(a.aperture, focus)
        if a.projection != "perspective":   # (every later camera move keeps it, with the new frustum's basis)
            r.set_projection(a.projection, height=a.ortho_height, lon_range=math.radians(a.lon_range), lat_range=math.radians(a.lat_range))
        if a.frames:
            if a.ripple:
                frames = ripple_frames(r, sc, a.frames, a.ripple, bool(a.temporal))
            else:
                frames = recolour_frames(r, sc, a.frames, a.recolour) if a.recolour else move_frames(r, sc, a.frames, a.move, a.width / a.height, a.shutter)
            for path, (rows, ms) in zip(frame_paths(a.out, a.frames), frames):
                r.save(path)
        else:
            rows, ms = r.render()
            r.save(a.out)  # the SaveFrameBuffer post-process stage (pipeline.go:215-235)
        if a.aov_dir:
            os.makedirs(a.aov_dir, exist_ok=True)
            imgs = aov_images(r.read_aov(T.AOV_GUIDE), r.read_aov(T.AOV_ALBEDO))
            for name, img in imgs.items():
                host_api.write_png(os.path.join(a.aov_dir, name + ".png"), img)
            if a.variance:
                np.save(os.path.join(a.aov_dir, "variance.npy"), r.read_aov(T.AOV_VARIANCE))
            if a.auto_exposure:
                e = r.read_exposure()
                with open(os.path.join(a.aov_dir, "exposure.json"), "w") as f:
                    json.dump({"valid": e["valid"], "n_metered": e["n_metered"], "avg": float(e["avg"]), "log2E": float(e["log2E"]), "E": float(e["E"]),
                               "histogram": e["histogram"].tolist()}, f)
    finally:
        r.close()
    print(f"{a.scene}: {sc.vertices.shape[0] // 3} triangles, {len(sc.mesh_instances)} instances, {len(sc.material_nodes)} material nodes; "
          f"compiled in {1e3 * (t1 - t0):.0f} ms; {a.width}x{a.height} @ {a.spp} spp on {len(devs)} tracer(s) rows={rows}: {ms:.1f} ms -> {frame_paths(a.out, a.frames)[-1] if a.frames else a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
