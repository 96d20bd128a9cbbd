"""Lifetimes of the handle's lazily allocated planes on the MI355X (polaris_amd/csrc/device_mem.h).

One tracer is taken through feature toggles and resizes that allocate, free, swap and re-allocate every filter plane; after every
sync its RGBA8 frame buffer, every AOV that can be read and the refusal of every AOV that cannot must equal, byte for byte, those
of a second tracer that was configured directly for that state and saw none of the earlier toggles and resizes.  A plane that
outlives its feature or frame size, is freed while in use, or is missing from
the set its feature frees (frame_sync.h) shows as a difference (or a fault) here.

Frames 24 x 16 and 40 x 12: 384 and 480 pixels, neither a multiple of the 256-thread workgroup.

The last two tests do the same for the handle's streams, events and inter-process events (DevStream / DevEvent in device_mem.h):
every kind is live when the handle is destroyed, and the ring of exported events shrinks and grows.  Every call in them succeeds."""
import dataclasses

import numpy as np
import pytest

from conftest import make_hip_tracer
from polaris_amd import ctypes_api as T
from test_gpu_denoise import sync, trace

pytestmark = pytest.mark.gpu

FRAME_A, FRAME_B = (24, 16), (40, 12)
SPP, BOUNCES = 2, 2
AOVS = {"guide": T.AOV_GUIDE, "albedo": T.AOV_ALBEDO, "denoised": T.AOV_DENOISED, "temporal": T.AOV_TEMPORAL, "prior": T.AOV_PRIOR,
        "variance": T.AOV_VARIANCE, "prior2": T.AOV_PRIOR2}
GBUFFER = {"guide", "albedo"}


def scenes_pair():
    """The Cornell box under the camera of frame A, and the same box with the eye moved (one scene for both frame sizes: a toggle
    or a resize must not need a new camera)."""
    from polaris_amd import scenes

    sc0 = scenes.SCENES["cornell"](FRAME_A[0] / FRAME_A[1])
    eye = (np.asarray(sc0.eye, np.float32) + np.array([0.02, 0.01, 0], np.float32)).astype(np.float32)
    return sc0, dataclasses.replace(sc0, eye=eye)


def set_camera(tr, sc):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.CameraData, sc)


def resize(tr, frame):
    from polaris_amd.tracer import ChangeType, UpdateMode

    tr.UpdateState(UpdateMode.Synchronous, ChangeType.FrameDimensions, frame)


def trace_sync(tr, frame, base):
    trace(tr, *frame, SPP, base=base, bounces=BOUNCES)
    sync(tr, *frame, SPP)


def snapshot(tr):
    """Frame-buffer bytes, and per AOV its bytes or its refusal (code and message)."""
    from polaris_amd.tracer import TracerError

    snap = {"framebuffer": tr.read_framebuffer().tobytes()}
    for name, which in AOVS.items():
        try:
            snap[name] = tr.read_aov(which).tobytes()
        except TracerError as e:
            snap[name] = ("refused", e.code, str(e))
    return snap


def check(step, got, want, readable, frame):
    """got == want byte for byte, exactly the AOVs in `readable` are planes of the frame's size, the others are refused alike."""
    assert set(got) == set(want)
    for name in got:
        assert got[name] == want[name], (step, name)
    for name in AOVS:
        if name in readable:
            assert isinstance(got[name], bytes) and len(got[name]) == frame[0] * frame[1] * 16, (step, name)
        else:
            assert got[name][:2] == ("refused", 2), (step, name, got[name])            # POLARIS_E_BAD_ARGUMENT
    assert len(got["framebuffer"]) == frame[0] * frame[1] * 4 and any(got["framebuffer"]), step


def fresh(sc, frame, *, variance=False, temporal=False, **options):
    tr = make_hip_tracer(sc, *frame, **options)
    tr.set_denoise(**T.DENOISE_DEFAULTS)
    if variance:
        tr.set_variance(**T.VARIANCE_DEFAULTS)
    if temporal:
        tr.set_temporal(**T.TEMPORAL_DEFAULTS)
    return tr


def fresh_snapshot(sc, frame, base, **features):
    tr = fresh(sc, frame, **features)
    try:
        trace_sync(tr, frame, base)
        return snapshot(tr)
    finally:
        tr.Close()


def test_planes_follow_toggles_and_resizes(built):
    sc0, sc1 = scenes_pair()
    tr = make_hip_tracer(sc0, *FRAME_A)
    ref = None
    try:
        tr.set_denoise(**T.DENOISE_DEFAULTS)                                         # 1. denoise on
        trace_sync(tr, FRAME_A, 3)
        check(1, snapshot(tr), fresh_snapshot(sc0, FRAME_A, 3), GBUFFER | {"denoised"}, FRAME_A)

        tr.set_variance(**T.VARIANCE_DEFAULTS)                                       # 2. variance on
        trace_sync(tr, FRAME_A, 4)
        check(2, snapshot(tr), fresh_snapshot(sc0, FRAME_A, 4, variance=True), GBUFFER | {"denoised", "variance"}, FRAME_A)

        tr.set_variance(0.0)                                                         # 3. variance off
        resize(tr, FRAME_B)                                                          # 4. the second frame
        tr.set_variance(**T.VARIANCE_DEFAULTS)                                       # 5. variance on
        tr.set_temporal(**T.TEMPORAL_DEFAULTS)                                       # 6. temporal reuse on
        trace_sync(tr, FRAME_B, 5)                                                   # 7.
        # the reference of the two temporal syncs: the same two syncs around the same camera move (the resize dropped any older
        # history, so this is the whole history)
        ref = fresh(sc0, FRAME_B, variance=True, temporal=True)
        trace_sync(ref, FRAME_B, 5)
        check(7, snapshot(tr), snapshot(ref), set(AOVS), FRAME_B)

        set_camera(tr, sc1)                                                          # 8. move the camera
        trace_sync(tr, FRAME_B, 6)                                                   # 9.
        set_camera(ref, sc1)
        trace_sync(ref, FRAME_B, 6)
        got = snapshot(tr)
        check(9, got, snapshot(ref), set(AOVS), FRAME_B)
        prior = np.frombuffer(got["prior"], np.float32).reshape(FRAME_B[1], FRAME_B[0], 4)
        assert (prior[..., 3] > 0).mean() > 0.5                                     # (the history is in play: m > 0 on most pixels)

        tr.set_temporal(0)                                                           # 10. temporal reuse off
        trace_sync(tr, FRAME_B, 7)                                                   # 11.
        check(11, snapshot(tr), fresh_snapshot(sc1, FRAME_B, 7, variance=True), GBUFFER | {"denoised", "variance"}, FRAME_B)

        resize(tr, FRAME_A)                                                          # 12. back to the first frame
        trace_sync(tr, FRAME_A, 8)                                                   # 13.
        check(13, snapshot(tr), fresh_snapshot(sc1, FRAME_A, 8, variance=True), GBUFFER | {"denoised", "variance"}, FRAME_A)
    finally:
        tr.Close()
        if ref is not None:
            ref.Close()


def test_destroy_with_every_plane_allocated(built):
    """Three create / upload / denoised-variance-temporal sync / destroy cycles in a row.  The history planes exist only after a
    camera move (set_camera swaps them in), hence the second sync; every cycle ends with all thirteen planes allocated."""
    sc0, sc1 = scenes_pair()
    snaps = []
    for _ in range(3):
        tr = fresh(sc0, FRAME_A, variance=True, temporal=True)
        try:
            trace_sync(tr, FRAME_A, 3)
            set_camera(tr, sc1)
            trace_sync(tr, FRAME_A, 4)
            snaps.append(snapshot(tr))
        finally:
            tr.Close()
    check("cycle", snaps[1], snaps[0], set(AOVS), FRAME_A)
    check("cycle", snaps[2], snaps[0], set(AOVS), FRAME_A)


def snapshot_with_instances(tr):
    """snapshot() plus the INSTANCE plane's bytes or its refusal (allowed with object motion in effect only)."""
    from polaris_amd.tracer import TracerError

    snap = snapshot(tr)
    try:
        snap["instance"] = tr.read_instance_plane().tobytes()
    except TracerError as e:
        snap["instance"] = ("refused", e.code, str(e))
    return snap


def test_object_motion_toggles_drop_history_and_instance_planes(built):
    """Denoise, variance guidance and temporal reuse on; the option object_motion goes 1 -> 0 -> 1 between syncs.  A toggle drops the
    history and the G-buffer and, turned off, the INSTANCE planes and the motion table; turned on after the upload it reads the
    instance matrices back from the device.  After every sync the tracer equals one configured directly for that state: the two syncs
    around the camera move with the option on from the start, then a new tracer under the moved camera with the option off, then on."""
    sc0, sc1 = scenes_pair()
    both = dict(variance=True, temporal=True)
    tr = fresh(sc0, FRAME_A, object_motion=1, **both)
    ref = fresh(sc0, FRAME_A, object_motion=1, **both)
    try:
        for step, (sc, base) in enumerate(((sc0, 3), (sc1, 4)), 1):                  # 1. sync; 2. move the camera, sync
            for t in (tr, ref):
                if sc is sc1:
                    set_camera(t, sc)
                trace_sync(t, FRAME_A, base)
            got = snapshot_with_instances(tr)
            check(step, got, snapshot_with_instances(ref), set(AOVS), FRAME_A)
            assert isinstance(got["instance"], bytes) and len(got["instance"]) == FRAME_A[0] * FRAME_A[1] * 4
        prior = np.frombuffer(got["prior"], np.float32).reshape(FRAME_A[1], FRAME_A[0], 4)
        assert (prior[..., 3] > 0).mean() > 0.5                                     # (the history is in play: m > 0 on most pixels)
        for step, (on, base) in enumerate(((0, 5), (1, 6)), 3):                      # 3. option off, sync; 4. option on, sync
            tr.set_option("object_motion", on)
            trace_sync(tr, FRAME_A, base)
            got = snapshot_with_instances(tr)
            new = fresh(sc1, FRAME_A, object_motion=on, **both)
            try:
                trace_sync(new, FRAME_A, base)
                check(step, got, snapshot_with_instances(new), set(AOVS), FRAME_A)
            finally:
                new.Close()
            if on:
                assert isinstance(got["instance"], bytes) and len(got["instance"]) == FRAME_A[0] * FRAME_A[1] * 4
            else:
                assert got["instance"][:2] == ("refused", 2) and "object_motion is off" in got["instance"][2]
            prior = np.frombuffer(got["prior"], np.float32)
            assert not prior.any()                                                  # (the toggle dropped the history: m = 0, PRIOR = 0)
    finally:
        tr.Close()
        ref.Close()


# ---- streams and events: every kind live, then released ---------------------------------------------------------------------
HANDLE_SPP = 4


def request(accumulated=0, spp=HANDLE_SPP):
    from oracle import pybind as ob

    return ob.make_request(*FRAME_A, spp=spp, bounces=BOUNCES, accumulated=accumulated)


def seeds(base):
    from polaris_amd import scenes

    return scenes.make_seeds(HANDLE_SPP, BOUNCES, base=base)


def test_destroy_with_every_kind_of_event_and_stream_live(built):
    """Two tracers with kernel timing on and four one-sample batches on four pipelines (the timer events cycle through the pool);
    `a` exports a ring of three (its inter-process events), merges `b` (one of a's merge-stream events enters b's reader list, moves
    to b's pool at b's next Trace and is taken out again by the next merge) and itself.  Three such cycles, closed in either order,
    give the same bytes."""
    sc0, _ = scenes_pair()
    req = request()
    snaps = []
    for cycle in range(3):
        a = make_hip_tracer(sc0, *FRAME_A, time_kernels=1, overlap=4, samples_per_batch=1)
        b = make_hip_tracer(sc0, *FRAME_A, time_kernels=1, overlap=4, samples_per_batch=1)
        try:
            a.ipc_export(3)
            a.Trace(req, seeds(3))
            b.Trace(req, seeds(4))
            a.MergeOutput(b, req)
            a.MergeOutput(a, req)
            b.Trace(req, seeds(5))
            a.MergeOutput(b, req)
            a.SyncFramebuffer(request(spp=3 * HANDLE_SPP))
            snaps.append({"framebuffer": a.read_framebuffer().tobytes(), "a.trace": a.read_accumulator(0).tobytes(),
                          "a.frame": a.read_accumulator(1).tobytes(), "b.trace": b.read_accumulator(0).tobytes()})
            assert a.kernel_ms("generate")[1] > 0
        finally:
            for tr in ((a, b) if cycle % 2 == 0 else (b, a)):
                tr.Close()
    assert any(snaps[0]["framebuffer"]) and any(snaps[0]["a.frame"])
    assert snaps[1] == snaps[0] and snaps[2] == snaps[0]


def test_exported_ring_shrinks_and_grows(built):
    """ipc_export(3), (1), (4) on one tracer with Traces in between: after every Trace its trace accumulator equals that of a plain
    tracer given the same seeds, and the three exports agree on whether they carry events."""
    sc0, _ = scenes_pair()
    req = request()
    tr, plain = make_hip_tracer(sc0, *FRAME_A), make_hip_tracer(sc0, *FRAME_A)
    try:
        has_event = []
        for depth, bases in ((3, (11, 12, 13)), (1, (14,)), (4, (15,))):
            has_event.append(int(T.IpcExport.from_buffer_copy(tr.ipc_export(depth)).has_event))
            for base in bases:
                tr.Trace(req, seeds(base))
                plain.Trace(req, seeds(base))
                got = tr.read_accumulator(0)
                assert got.any() and got.tobytes() == plain.read_accumulator(0).tobytes(), (depth, base)
        assert has_event[1] == has_event[0] and has_event[2] == has_event[0]
    finally:
        tr.Close()
        plain.Close()
