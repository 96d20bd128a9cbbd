/*
 * polaris_hip.h -- C ABI of the MI355X (gfx950) tracer backend for polaris.
 *
 * This is the drop-in boundary: exactly what a Go package `tracer/hip` implementing
 * tracer.Tracer (reference tracer/tracer.go:80-111) binds through cgo, replacing
 * tracer/opencl (+ tracer/opencl/device).  Plain pointers and sizes only; no C++/torch
 * types; every function returns 0 on success or a POLARIS_E_* code, never throws/aborts.
 * INTEGRATION.md shows the Go side.
 *
 * Method-by-method correspondence (reference file:line -> entry point):
 *   device.GetPlatformInfo / SelectDevices, Speed estimate
 *       tracer/opencl/device/platform.go, device.go:209-222  -> polaris_hip_device_count/_info
 *   opencl.NewTracer + Tracer.Init   tracer/opencl/tracer.go:58-117      -> polaris_hip_create
 *   Tracer.Close                     tracer/opencl/tracer.go:120-145     -> polaris_hip_destroy
 *   Tracer.UpdateState(FrameDimensions)  tracer.go:169-171 -> buffers.go:127-174 Resize
 *                                                                        -> polaris_hip_resize
 *   Tracer.UpdateState(SceneData)    tracer.go:172-174 -> buffers.go:180-201 UploadSceneData
 *                                                                        -> polaris_hip_upload_scene
 *   Tracer.UpdateState(CameraData)   tracer.go:175-179                   -> polaris_hip_set_camera
 *   Tracer.Trace                     tracer.go:194-247 + pipeline.go:94-213 -> polaris_hip_trace
 *   Tracer.MergeOutput               tracer.go:279-286, resources.go:108-124 -> polaris_hip_merge
 *   Tracer.SyncFramebuffer           tracer.go:250-276, resources.go:344-360 -> polaris_hip_sync_framebuffer
 *   SaveFrameBuffer's ReadData       pipeline.go:226-232                 -> polaris_hip_read_framebuffer
 *   errors                           tracer/opencl/errors.go:5-22        -> POLARIS_E_* + polaris_hip_last_error
 *
 * Threading: any entry point may be called from any OS thread (goroutines migrate); each
 * call binds the handle's device.  Calls on ONE handle are serialised by a per-handle mutex;
 * polaris_hip_merge(dst, src, ..) may be called concurrently from several threads onto one
 * dst (renderer/default.go:188-191 does exactly that) and with src == dst.
 * Ownership: the library copies everything it needs before returning; no caller pointer is
 * retained (cgo rule).
 */
#ifndef POLARIS_HIP_H
#define POLARIS_HIP_H

#include "polaris_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  2: + reset_epoch / wait_reset, kernel_symbol, shade_counts.  3: + ipc_export / ipc_open / ipc_close / merge_ipc / merge_slot /
 * trace_slot (additions only: older callers keep working).  4: PolarisIpcExport carries one event handle PER RING SLOT (the blob grows from 352
 * to 544 bytes; ipc_open refuses a blob of another version); PolarisBvhBuildInput grew by `algorithm` (64 -> 72 bytes) and polaris_hip_build_bvh's
 * default for a zero-initialised caller changed from the linear BVH to the binned-SAH builder.  5: + device_identity / can_access_peer /
 * peer_info / merge_counts (which GPU a tracer really runs on, and which branch every merge took: what a multi-GPU bench line needs to prove
 * itself); PolarisIpcExport carries the exporting GPU's PCI bus id (544 -> 576 bytes); PolarisBvhBuildInput LEADS with `struct_size`
 * (72 -> 80 bytes): a caller built against another layout is refused instead of being read past its end.  Still 5: + update_instances,
 * + update_vertices / PolarisVertexUpdate, + update_materials / PolarisMaterialUpdate / update_texture and the record kinds
 * POLARIS_REC_TRIS / POLARIS_REC_SHADING, + set_lens / PolarisLensParams, + set_shutter / PolarisShutterParams, + set_projection / PolarisProjectionParams
 * (additions only: older callers keep working). */
#define POLARIS_HIP_ABI_VERSION 5

/* status codes (0 = ok).  The first three mirror tracer/opencl/errors.go sentinels. */
#define POLARIS_OK                0
#define POLARIS_E_NO_SCENE_DATA   1  /* ErrNoSceneData: Trace/Sync before a scene upload (tracer.go:203-205,254-256) */
#define POLARIS_E_BAD_ARGUMENT    2  /* null pointer, block outside frame, too many bounces, short seed list */
#define POLARIS_E_NO_DEVICE       3  /* device index out of range / no HIP device */
#define POLARIS_E_DEVICE          4  /* a HIP runtime call failed; text in last_error */
#define POLARIS_E_BAD_SCENE       5  /* scene arrays inconsistent (index out of range, BVH deeper than the traversal stack) */
#define POLARIS_E_UNSUPPORTED     6  /* e.g. merge between handles that cannot reach each other */
#define POLARIS_E_TIMEOUT         7  /* polaris_hip_wait_reset: the awaited Reset stage did not arrive within 120 s */

typedef struct polaris_hip_tracer polaris_hip_tracer; /* opaque */

int polaris_hip_abi_version(void);

/* Device enumeration.  Speed estimate of the reference = compute_units * clock_mhz / 1000
 * (tracer/opencl/device/device.go:219); the Go side computes it from these two numbers. */
int polaris_hip_device_count(void);
int polaris_hip_device_info(int index, char name[256], uint32_t *compute_units, uint32_t *clock_mhz,
                            uint64_t *global_mem_bytes);

/* Which physical GPU a HIP device index of THIS process is.  Device indices are per process: a launcher that masks every rank to one
 * visible device (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES per rank) makes index 0 a different GPU in every rank, and a
 * misconfigured one makes it the SAME GPU in all of them -- the PCI bus id and the UUID tell which.  The reference names its devices by
 * the OpenCL device name and has ONE process see them all (tracer/opencl/device/platform.go, renderer/default.go:204-256: one tracer
 * per enumerated device); with one process per GPU the identity has to travel with the numbers (bench.py: config.devices,
 * config.distinct_gpus).  The caller sets struct_size = sizeof(PolarisDeviceIdentity). */
typedef struct PolarisDeviceIdentity {
	uint32_t struct_size;
	int32_t hip_index;
	char pci_bus_id[32];   /* hipDeviceGetPCIBusId, e.g. "0000:05:00.0" */
	uint8_t uuid[16];      /* hipDeviceGetUuid; all zero if the runtime reports none */
	uint32_t compute_units, clock_mhz;
	uint64_t global_mem_bytes;
	char name[64];         /* hipDeviceProp_t.name, truncated */
	char gcn_arch[32];     /* hipDeviceProp_t.gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
} PolarisDeviceIdentity;
int polaris_hip_device_identity(int index, PolarisDeviceIdentity *out);
/* hipDeviceCanAccessPeer(device, peer_device) for two device indices of this process: *can = 1 / 0 (0 for device == peer_device, as HIP
 * answers).  What decides between the direct peer read and the staged copy of polaris_hip_merge (tracer/opencl/tracer.go:279-286: the
 * reference's devices share one context and the runtime migrates the buffer). */
int polaris_hip_can_access_peer(int device, int peer_device, int *can);

int polaris_hip_create(int device_index, polaris_hip_tracer **out);
void polaris_hip_destroy(polaris_hip_tracer *h);

/* Text of the last error on this handle (or, with h == NULL, of the calling thread's last
 * failed create/device call).  Valid until the next call on the same handle/thread. */
const char *polaris_hip_last_error(polaris_hip_tracer *h);

/* (Re)allocate every frame-sized buffer; clears the frame accumulator. */
int polaris_hip_resize(polaris_hip_tracer *h, uint32_t frame_w, uint32_t frame_h);

/* Validate, re-lay-out for traversal and upload the scene.  Everything is copied.  With temporal reuse on, the history is dropped
 * (it saw the old scene) -- unless the option "object_motion" is in effect: then the upload is to the history what a set_camera is
 * (the planes of a temporal sync under the old scene become the history, with the old scene's instance table), and the history is
 * kept if the new scene is compatible with it: the same num_mesh_instances, the same mesh_index per instance and the same
 * num_triangles.  Only inv_transform may differ between compatible scenes as far as the library can tell: vertex and material edits
 * under an unchanged topology are the caller's responsibility (upload such a scene with the option off, or drop the history with
 * polaris_hip_set_temporal(max_history = 0) first). */
int polaris_hip_upload_scene(polaris_hip_tracer *h, const PolarisSceneView *scene);

/* eye[3]; frustum[16] = corner rays TL, TR, BL, BR as float4 (scene.Camera.Frustrum). */
int polaris_hip_set_camera(polaris_hip_tracer *h, const float eye[3], const float frustum[16]);

/* Thin-lens camera: depth of field (no reference counterpart; the reference's only PrimaryRayGenerator is the pinhole).  Off by
 * default and while u = v = 0: every Trace, tap and sync then allocates and launches exactly what it did, under the same kernel
 * symbols.  With it on, the camera rays of a Trace and of polaris_hip_tap_primary come from k_generate_lens: d is the pinhole's unit
 * direction (same arithmetic, same first draw of the camera PRNG), the stream's SECOND draw is mapped to the unit disk (Shirley-Chiu
 * concentric map) as (lx, ly), the ray starts at the lens point eye + lx u + ly v and passes through the pinhole ray's point on the
 * plane of focus, eye + d focus_distance / (d . axis).  A direction with d . axis <= 0 keeps its pinhole ray.  DESIGN.md 10h has
 * the exact float32 arithmetic.  The vectors are explicit, as set_camera's eye and frustum are: the library derives nothing.
 * polaris_hip_set_camera does NOT touch them -- a caller that moves the camera sets the lens again (the layers above do it for
 * their callers: polaris_amd/tracer.py set_lens, the host layer's CameraData.lens_radius).
 * What stays pinhole: the G-buffer (GUIDE, ALBEDO, the INSTANCE plane) is still one ray from the eye through the pixel centre, and
 * the temporal reprojection projects with the pinhole camera -- a strongly defocused region is filtered against sharp guide edges.
 * A call that changes any byte of the parameters drops the temporal history (as max_history = 0 does; the G-buffer stays) and the
 * caller restarts accumulation, as after a set_camera; a call with identical bytes does nothing.
 * POLARIS_E_BAD_ARGUMENT, state unchanged: null params, another struct_size, a float that is not finite, an entry of u or v above
 * 2^30 in magnitude, and with the lens on a focus_distance outside [1e-6, 1e30] or |axis|^2 outside [0.998, 1.002]. */
typedef struct PolarisLensParams {
	uint32_t struct_size;     /* = sizeof(PolarisLensParams) = 44 */
	float    focus_distance;  /* distance of the plane of focus from the eye, measured along `axis` */
	float    axis[3];         /* unit view axis (world space) */
	float    u[3], v[3];      /* the two world-space vectors that span the aperture: a lens point is eye + lx u + ly v,
	                             (lx, ly) uniform in the unit disk.  |u| = |v| = aperture radius for a round lens.
	                             u = v = 0 (all six floats zero): the lens is OFF, nothing else is looked at */
} PolarisLensParams;
int polaris_hip_set_lens(polaris_hip_tracer *h, const PolarisLensParams *p);

/* Camera shutter: motion blur of the camera and focus pulls inside one accumulation (no reference counterpart).  Off by default and
 * while enabled = 0: every Trace, tap and sync then launches exactly what it did, under the same kernel symbols.  The state at
 * shutter OPEN is what polaris_hip_set_camera and polaris_hip_set_lens hold; this struct is the state at shutter CLOSE.  With it on,
 * the camera rays of a Trace and of polaris_hip_tap_primary come from k_generate_shutter<LENS>: after the sub-pixel draw (and, with the
 * lens on, the lens draw) the camera PRNG's next draw gives the ray its time t in [0, 1), and the ray is generated by the camera
 * whose eye, corner rays and (lens on) lens are a + (b - a) t per component between open a and close b -- uniform over the interval,
 * corners and axis blended linearly (the axis is not renormalised; a caller who turns far inside one exposure subdivides it).  A close
 * state equal to the open one gives the rays of the shutter-off generator bit for bit (a -0 entry becomes +0).  DESIGN.md 10j has the
 * exact float32 arithmetic.
 * The close state belongs to the open state it was set after: polaris_hip_set_camera switches the shutter off, and so does a
 * polaris_hip_set_lens that changes a byte (one with identical bytes does nothing, as before).  The order of calls is therefore camera,
 * lens, shutter; the layers above re-apply it for their callers.
 * What stays at the open camera: the G-buffer (GUIDE, ALBEDO, the INSTANCE plane) and the temporal reprojection, which are pinhole at
 * the open camera as they are under a lens.  Only the camera moves: instances and deforming meshes are not blurred.
 * A call that changes the state drops the temporal history (as a changed lens does; the G-buffer stays) and the caller restarts
 * accumulation; a call whose bytes equal the stored ones does nothing, and any two off states are equal.
 * POLARIS_E_BAD_ARGUMENT, state unchanged: a null handle or params, another struct_size, enabled > 1, no camera set yet; with
 * enabled = 1 an eye1 or frustum1 float that is not finite, and WHILE THE LENS IS ON the rules of polaris_hip_set_lens for the close
 * lens: ten finite floats, entries of u1 / v1 at most 2^30 in magnitude, focus_distance1 within [1e-6, 1e30], |axis1|^2 within
 * [0.998, 1.002] (u1 = v1 = 0 is allowed: the aperture closes over the interval).  With the lens off the ten lens floats are not
 * looked at. */
typedef struct PolarisShutterParams {
	uint32_t struct_size;      /* = sizeof(PolarisShutterParams) = 124 */
	uint32_t enabled;          /* 0 = off (default): nothing else is looked at.  1 = on.  Anything else: BAD_ARGUMENT */
	float    eye1[3];          /* the eye at shutter close */
	float    frustum1[16];     /* the corner rays TL, TR, BL, BR at shutter close, as set_camera's */
	float    focus_distance1;  /* the lens at shutter close: looked at only while the lens is on */
	float    axis1[3], u1[3], v1[3];
} PolarisShutterParams;
int polaris_hip_set_shutter(polaris_hip_tracer *h, const PolarisShutterParams *p);

/* Camera projection: orthographic and equirectangular (latitude-longitude) cameras beside the perspective frustum of
 * polaris_hip_set_camera (no reference counterpart).  Off by default and while kind = 0: nothing else in the struct is looked at, any
 * two off states are equal, and every Trace, tap, G-buffer and sync launches exactly what it did, under the same kernel symbols.
 * The eye is polaris_hip_set_camera's; its frustum stays stored and is not read while kind != 0.  The view basis is explicit, as the
 * lens' vectors are: the library derives nothing, polaris_hip_set_camera does NOT touch it, and a caller that turns the camera sets the
 * projection again (the layers above do it for their callers).
 * With tx, ty the sample's frame coordinates in [0, 1) (k_generate's: pixel + tent-filtered offset, times 1 / W and 1 / H):
 *   ORTHOGRAPHIC     the ray starts at eye + right (2 tx - 1) half_width + up (1 - 2 ty) half_height and runs along `axis`, verbatim;
 *   EQUIRECTANGULAR  the ray starts at the eye; lon = (tx - 0.5) lon_range, lat = (0.5 - ty) lat_range, and its direction is
 *                    normalise(axis cos(lat) cos(lon) + right cos(lat) sin(lon) + up sin(lat)).
 * The camera rays of a Trace and of polaris_hip_tap_primary come from k_generate_proj<kind>; the G-buffer casts the same ray through the
 * pixel centre and the temporal reprojection inverts the same projection (GUIDE t under ORTHOGRAPHIC is the distance along the axis).
 * There is no wrap across the equirectangular seam.  DESIGN.md 10n has the exact float32 arithmetic.
 * A call that changes the state drops the G-buffer and the temporal history (the planes stay) and the caller restarts accumulation; a
 * call whose bytes equal the stored ones does nothing.  polaris_hip_set_camera under a projection is an ordinary camera move: the
 * history survives a translation of the eye.
 * POLARIS_E_BAD_ARGUMENT, state unchanged: a null handle or params, another struct_size, kind > 2; with kind != 0 also: no camera set
 * yet, any of the 13 floats not finite, |axis|^2, |right|^2 or |up|^2 outside [0.998, 1.002], a pairwise |dot| above 1e-3,
 * ORTHOGRAPHIC with half_width or half_height outside [1e-6, 1e30], EQUIRECTANGULAR with lon_range outside [1e-3, 6.2831855] or
 * lat_range outside [1e-3, 3.1415927] (the two fields of the other kind must only be finite), the lens on or the shutter on.  While a
 * projection is on, a polaris_hip_set_lens that would switch the lens on and a polaris_hip_set_shutter with enabled = 1 are refused. */
enum { POLARIS_PROJECTION_PERSPECTIVE = 0, POLARIS_PROJECTION_ORTHOGRAPHIC = 1, POLARIS_PROJECTION_EQUIRECTANGULAR = 2 };
typedef struct PolarisProjectionParams {
	uint32_t struct_size;     /* = sizeof(PolarisProjectionParams) = 60 */
	uint32_t kind;            /* POLARIS_PROJECTION_*; 0 = off (default): nothing else is looked at */
	float    axis[3], right[3], up[3]; /* orthonormal view basis, world space: +axis forward, +right to image right, +up to image top */
	float    half_width, half_height;  /* ORTHOGRAPHIC: half extents of the window through the eye, world units */
	float    lon_range, lat_range;     /* EQUIRECTANGULAR: radians spanned by the frame's width and height */
} PolarisProjectionParams;
int polaris_hip_set_projection(polaris_hip_tracer *h, const PolarisProjectionParams *p);

/* Tunables (not part of the reference interface).  Keys:
 *   "samples_per_batch"  samples traced concurrently as one wavefront batch (default: auto)
 *   "exact_accumulate"   1 = add every contribution straight into the trace accumulator in
 *                        the reference's order (forces one sample per batch; bit-exact with
 *                        the CPU oracle), 0 = per-path radiance + ordered resolve (default)
 *   "packet_primary"     1 = wave-packet traversal for primary rays, 0 = per-ray, -1 = by scene
 *                        (default: packets for single-instance scenes of up to 32 K triangles,
 *                        except where the tiny-scene mode keeps the triangle records in LDS)
 *   "lds_tris"           NEXT upload, tiny-scene mode: triangle records kept in LDS beside the tree
 *                        (default -1: as many as fit half a CU's LDS, none if that is under half
 *                        of them; 0 = none)
 *   "tiny_one"           NEXT upload: 0 = the general tiny-scene kernel even where the variant for
 *                        single-instance scenes with bounding boxes applies (default 1)
 *   "time_kernels"       1 = bracket every kernel with HIP events (polaris_hip_kernel_ms)
 *   "moments"            1 = the batch epilogue also adds L_s^2 of every sample (L = Rec. 709 luminance, csrc/variance.h) to
 *                        the trace accumulator's .w, and merges onto this tracer add .w too (the input of
 *                        polaris_hip_set_variance); .rgb are the same bit for bit.  Default 0.  POLARIS_E_UNSUPPORTED together
 *                        with "exact_accumulate" = 1 (in either order: that mode has no per-sample radiance); 0 is
 *                        POLARIS_E_BAD_ARGUMENT while variance guidance is on
 *   "object_motion"      0 (default) or 1: temporal reuse (polaris_hip_set_temporal) survives an upload_scene that only moves mesh
 *                        instances.  The first-hit G-buffer gains an INSTANCE plane (polaris_hip_read_instance_plane), the history
 *                        carries the instance table it was seen with, and the reprojection takes a first hit of instance k back
 *                        through inverse(inv_transform_history[k]) . inv_transform_now[k] before it projects it into the history
 *                        camera; a history tap must show the same instance.  In effect only while max_history > 0.
 *                        The tracer keeps a host copy of the scene's instance table (mesh_index, inv_transform, num_triangles)
 *                        from every upload_scene made with the option on.  Turned on after the scene, it takes the matrices
 *                        from the uploaded instance records: camera moves reuse the history at once, but the first upload_scene
 *                        after that still drops it (the old scene's mesh indices were not kept); set it before the scene.
 *                        Changing it drops the history and invalidates the G-buffer.  It never changes an accumulator or a
 *                        counter; off, no device memory is allocated and no kernel launched for it
 *   "vertex_motion"      0 (default) or 1, anything else POLARIS_E_BAD_ARGUMENT: temporal reuse survives polaris_hip_update_vertices
 *                        (DESIGN.md 10k).  In effect only while "object_motion" is in effect, the option is 1 and the scene was uploaded
 *                        with "vertex_update" on.  Then update_vertices is to the history what polaris_hip_update_instances is: the
 *                        planes of a temporal sync under the old vertices join the history, which stays; the first-hit G-buffer gains
 *                        a HIT plane (polaris_hip_read_hit_plane); just before the first update that would overwrite the vertices a
 *                        history was seen with, they are copied on the device ([3 num_triangles] float4, scene order); and the
 *                        reprojection takes a first hit whose triangle changed to the point of the old triangle at the same
 *                        barycentrics, through inverse(inv_transform_history[k]), before it projects it into the history camera.  A
 *                        triangle whose nine coordinates did not change takes "object_motion"'s path bit for bit.  update_materials,
 *                        update_texture and an incompatible upload_scene drop the history as without it.  Changing the value drops
 *                        the history and invalidates the G-buffer, as changing "object_motion" does; setting the same value does
 *                        nothing.  It never changes an accumulator or a counter; off or without effect, every upload, update, sync
 *                        and G-buffer allocates and launches exactly what it does without the option
 *   "bloom_fused"        0 (default) or 1, anything else POLARIS_E_BAD_ARGUMENT: with polaris_hip_set_bloom in effect, 1 runs every
 *                        pyramid level of at most 1024 pixels, down and up, in one launch (k_bloom_tail); 0 runs one launch per
 *                        level.  An A/B switch: the pyramid's values are the same bit for bit.  Off by default: measured on an
 *                        MI355X it saves 0.6 us of 32 at 512 x 512 and costs 3 us of 39 at 1024 x 1024
 *   "guide_specular"    0 (default) .. 8, anything else POLARIS_E_BAD_ARGUMENT: the number N of delta interactions the G-buffer's
 *                        guide ray follows.  With N > 0 a pixel whose hit is a CONDUCTOR or DIELECTRIC leaf -- both
 *                        delta BxDFs: a mirror, smooth glass -- continues in the mirror direction, or through the glass (refracted
 *                        wherever refraction exists, reflected on total internal reflection), up to N times, and GUIDE / ALBEDO /
 *                        INSTANCE describe the first surface it does not follow through (see the planes below): the filter and the
 *                        reprojection then see what the pixel shows, not the smooth surface in front of it.  Every link is the first
 *                        hit's own walk again (PRNG state (p, p), no path flags), the continuation ray is the shade kernels'.  A
 *                        chain that is exhausted (N links followed, a delta leaf again) describes that delta surface with the
 *                        accumulated distance and albedo; a delta direction that is not finite, all zero or beyond 2^10 in a
 *                        component ends the chain at its surface.  0 is the first hit: k_gbuffer with its arguments, every plane
 *                        bit for bit.  Changing the value invalidates the G-buffer and drops the temporal history, as changing
 *                        "object_motion" does; setting the same value does nothing.  It never changes an accumulator or a counter
 *   "instance_update"   0 (default) or 1, applies to the NEXT upload_scene: the upload keeps what polaris_hip_update_instances
 *                        needs (the top-level tree as a refit schedule, the triangle list of every mesh, host copies of the
 *                        emissive list and the packed light geometry).  Off, an upload keeps nothing extra: every
 *                        code path, allocation and launch is what it is without the option
 *   "vertex_update"      0 (default) or 1, applies to the NEXT upload_scene: the upload keeps everything "instance_update" keeps (so
 *                        polaris_hip_update_instances is accepted too) plus what polaris_hip_update_vertices needs: the slot -> scene
 *                        triangle map and the mesh trees as a refit schedule.  Off, an upload allocates, copies
 *                        and launches exactly what it does without the option
 *   "overlap"            batches in flight on separate streams (1-8, default 4)
 *   "max_leaf_tris"      applies to the NEXT upload_scene: triangle leaves with more triangles
 *                        than this are subdivided where a surface-area split pays (default -1:
 *                        2 up to 32 K triangles, 4 above; 0 = keep the caller's leaves).  Never
 *                        changes a result: DESIGN.md 2 (HBM data layout)
 *   "shade_prefilter"    1 (default): the shade kernels retire, before they shade a hit, the rays whose whole effect is a count --
 *                        a ray that left a scene without a background, and a ray that Russian roulette rejects on a hit whose
 *                        material cannot end in an emitter (the roulette reads only the carried throughput and the ray's third
 *                        PRNG draw).  0: every ray goes through the full shading code (k_shade_wave still queues them).  Never
 *                        changes an accumulator or a counter: it exists for the A/B and the equality tests
 *   "shade_wave_from"    first bounce shaded by k_shade_wave (persistent waves over groups of 8 chunks); never bounce 0.  -1 (default):
 *                        min_bounces_for_rr + 1 -- or min_bounces_for_rr, the bounce where Russian roulette starts, when
 *                        "shade_prefilter" is on, some shading class of the scene cannot emit and a full batch of the Trace holds at
 *                        least 8 such groups per compute unit.  Never changes an accumulator or a counter
 *   further A/B switches of the kernels ("traversal", "node_mode", "packet_shadow", "shade_wave",
 *   "shade_wave_from", "shade_sort", "shade_wgs_per_cu", "stage_lds", "trace_wgs_per_cu", "trace_grid", "hit12", "o12", "ipc_staged"): see
 *   DESIGN.md 3.  Apart from "exact_accumulate" (the order of the float sums) no option changes a
 *   result; an unknown key is POLARIS_E_BAD_ARGUMENT.  The batch size chosen automatically
 *   ("samples_per_batch" = 0) is clamped by the FREE device memory, and with it the order of the
 *   batched per-pixel float sums: non-exact output is bit-reproducible on one machine state, not
 *   across machines (exact_accumulate = 1 is, everywhere). */
int polaris_hip_set_option(polaris_hip_tracer *h, const char *key, int64_t value);

/*
 * Tracer.Trace: clears the frame accumulator if req->accumulated_samples == 0, clears the
 * trace accumulator, then traces req->samples_per_pixel samples over rows
 * [block_y, block_y+block_h).  The host PRNG draws of the reference (Go math/rand: one per
 * sample, tracer.go:222, plus one per bounce, pipeline.go:146) are passed in explicitly:
 *   seeds[s*(1+num_bounces)]       camera seed of sample s
 *   seeds[s*(1+num_bounces)+1+b]   shade seed of bounce b of sample s
 * n_seeds >= samples_per_pixel*(1+num_bounces).  Blocks until the device is done (the
 * reference's Trace is synchronous: every launch ends in clFinish, device/kernel.go:124).
 * stats may be NULL.
 */
int polaris_hip_trace(polaris_hip_tracer *h, const PolarisBlockRequest *req, const uint32_t *seeds,
                      size_t n_seeds, PolarisTraceStats *stats);

/* Tracer.MergeOutput: dst.frameAccumulator[rows of req] += src.traceAccumulator[rows of req].
 * Asynchronous like the reference (Exec1DNoWait, resources.go:119): queued on dst's MERGE stream -- the
 * stream that owns the frame accumulator (the Reset stage, merges) -- under a mutex of its own, so it does
 * not wait for a Trace running on dst (renderer/default.go:188-191 merges from the secondaries' goroutines
 * while the primary still traces); completed by polaris_hip_sync_framebuffer(dst).  The caller orders it
 * after src's Trace (synchronous) and after the START of dst's Trace of the same frame, which clears the
 * frame accumulator when accumulated_samples == 0 (the reference races there; polaris_amd/host/renderer.cpp
 * waits).  src may live on another GPU of the same process (peer access over xGMI, falling back to a
 * staged peer copy).  src must not be handed its next Trace's rows to overwrite before this merge has read them: the
 * library orders that on the device (src's next Trace waits for an event dst's merge stream records behind the read), so
 * the host need not sync in between. */
int polaris_hip_merge(polaris_hip_tracer *dst, polaris_hip_tracer *src, const PolarisBlockRequest *req);

/* One-process-per-GPU variant of the same exchange (bench.py under torch.distributed):
 * export copies the block's rows of the trace accumulator (block_h*frame_w float4) to a device
 * buffer the caller owns; merge_device adds such a strip, resident on dst's device, into
 * dst's frame accumulator. */
int polaris_hip_export_block(polaris_hip_tracer *h, const PolarisBlockRequest *req, void *device_dst);
int polaris_hip_merge_device(polaris_hip_tracer *dst, const void *device_rows, const PolarisBlockRequest *req);

/*
 * Cross-PROCESS merge: peer reads over HIP IPC (one process per GPU, the driver's launch contract).
 *
 * The reference gives all devices ONE shared OpenCL context, so the primary's aggregateAccumulator kernel reads a
 * secondary's traceAccumulator cl_mem directly (renderer/default.go:225-229, tracer/opencl/tracer.go:279-286,
 * resources.go:108-124).  Across processes the same read goes through an IPC mapping of the secondary's buffer:
 *
 *   secondary                                             primary
 *   polaris_hip_ipc_export(h, depth, &blob)   -- once, after resize; the blob is plain bytes for any channel -->
 *                                                         polaris_hip_ipc_open(dst, &blob, &peer)
 *   polaris_hip_trace(h, ..)      writes ring slot s = polaris_hip_trace_slot(h)
 *      -- "frame f is in slot s" (a host message AFTER Trace returned: Trace is synchronous) -->
 *                                                         polaris_hip_merge_ipc(dst, peer, s, req)   k_aggregate over the
 *                                                             peer-mapped rows, on dst's merge stream (xGMI peer read)
 *
 * ipc_export turns the tracer's trace accumulator into a RING of `depth` frame-sized buffers (1..POLARIS_IPC_MAX_DEPTH):
 * every later Trace writes the next slot, so the primary may still be reading frame f's rows while the secondary traces
 * frame f + 1 -- no copy, no staging strip.  The caller's protocol must guarantee that the primary has finished reading a
 * slot (its merge completed: sync_framebuffer) before the secondary's Trace comes round to it again; with the exchange one
 * frame behind the tracing that needs depth 3 (polaris_amd/distributed.py: PeerExchange states the argument).  The blob
 * also carries one inter-process event PER RING SLOT, recorded at the end of the Trace that wrote the slot; merge_ipc(slot)
 * makes the merge stream wait for that slot's event (device-side ordering on top of the host message; has_event = 0 if the
 * runtime could not export them).  Because a slot's event is only re-recorded when a Trace comes round to the slot again --
 * which the protocol above rules out while the slot may still be read -- the wait names exactly the Trace whose rows are
 * read, however far the secondary has run ahead (ABI 3 had one event for the whole ring, re-recorded by every Trace).  A resize
 * invalidates the export: peers close, the tracer exports again.  hipIpcOpenMemHandle cannot open a handle in the process
 * that created it: tracers of ONE process use polaris_hip_merge / polaris_hip_merge_slot.
 */
#define POLARIS_IPC_MAX_DEPTH 4
typedef struct PolarisIpcExport {
	uint32_t abi_version, depth, frame_w, frame_h;
	int32_t device;     /* HIP device index in the exporting process */
	uint32_t pid;       /* exporting process (diagnostics; opening in the same process is refused) */
	uint32_t has_event; /* 1: `event[i]` holds a hipIpcEventHandle_t for every slot i < depth */
	uint32_t reserved;
	uint8_t mem[POLARIS_IPC_MAX_DEPTH][64];   /* hipIpcMemHandle_t per ring slot */
	uint8_t event[POLARIS_IPC_MAX_DEPTH][64]; /* hipIpcEventHandle_t per ring slot: recorded at the end of the Trace that wrote the slot */
	char pci_bus_id[32];                      /* ABI 5: the exporting GPU (device indices mean nothing across processes; "" if unknown) */
} PolarisIpcExport;
typedef struct polaris_hip_peer polaris_hip_peer; /* opaque: another process's trace accumulator ring, mapped here */

int polaris_hip_ipc_export(polaris_hip_tracer *h, uint32_t depth, PolarisIpcExport *out);
int polaris_hip_ipc_open(polaris_hip_tracer *dst, const PolarisIpcExport *peer_export, polaris_hip_peer **out);
int polaris_hip_ipc_close(polaris_hip_tracer *dst, polaris_hip_peer *peer); /* waits for dst's merge stream first */
/* What a mapped ring really is (ABI 5): the exporter's GPU by PCI bus id, whether that is dst's OWN GPU (the mapping is then a second
 * mapping of local memory: ranks sharing a device, the one-GPU tests) or ANOTHER one (reads cross xGMI / PCIe), the exporter's GPU as a
 * device index of this process (-1: not visible here, e.g. under a per-rank visibility mask) and hipDeviceCanAccessPeer towards it
 * (-1: unknown).  ipc_open REFUSES (POLARIS_E_UNSUPPORTED) a ring on another GPU that this process cannot see at all -- there is no way to
 * tell whether the mapping would be reachable, and a kernel that reads an unreachable mapping faults the GPU; the caller falls back to
 * its strip transfers -- and marks every ring it does not KNOW to be reachable (a visible GPU without peer access, a failed query, no bus
 * id on either side) for the staged path (POLARIS_MERGE_IPC_STAGED; option "ipc_staged" = 1 forces that path for the peers opened
 * afterwards: a testing aid).  The caller sets struct_size. */
typedef struct PolarisPeerInfo {
	uint32_t struct_size;
	uint32_t pid;             /* exporting process */
	int32_t exporter_device;  /* its HIP device index in THAT process */
	int32_t local_device;     /* the same GPU as a device index of this process; -1 = not visible here */
	int32_t same_device;      /* 1: the ring lives on dst's own GPU; 0: on another GPU; -1: unknown (no bus id on either side) */
	int32_t can_access_peer;  /* hipDeviceCanAccessPeer(dst's device, local_device); -1 = unknown */
	uint32_t depth, has_events;
	char pci_bus_id[32];
	int32_t staged;           /* 1: merges from this ring go through the staging strip (not known to be reachable, or forced); 0: read where it lies */
	int32_t reserved;
} PolarisPeerInfo;
int polaris_hip_peer_info(polaris_hip_peer *peer, PolarisPeerInfo *out);
/* dst.frameAccumulator[rows of req] += peer.traceAccumulator ring[slot][rows of req]; asynchronous on dst's merge stream
 * like polaris_hip_merge, completed by polaris_hip_sync_framebuffer(dst). */
int polaris_hip_merge_ipc(polaris_hip_tracer *dst, polaris_hip_peer *peer, uint32_t slot, const PolarisBlockRequest *req);
/* The ring slot the last Trace wrote (0 without a ring; a Trace that fails before it has queued anything leaves it alone),
 * and polaris_hip_merge from a given slot of a tracer of THIS process (a primary that merges its own block one frame late
 * reads the slot of that frame, not the newest).  Like polaris_hip_merge, a merge_slot with src != dst is fenced on the
 * device against src's next Trace. */
int polaris_hip_trace_slot(polaris_hip_tracer *h, uint32_t *slot);
int polaris_hip_merge_slot(polaris_hip_tracer *dst, polaris_hip_tracer *src, uint32_t slot, const PolarisBlockRequest *req);

/* Which branch the merges onto `dst` took since it was created (ABI 5), counted per call under dst's merge lock:
 *   LOCAL         polaris_hip_merge / _merge_slot, source on dst's own device (src == dst included)
 *   PEER_ACCESS   ... source on another GPU of this process, read directly (hipDeviceEnablePeerAccess: xGMI peer read)
 *   STAGED        ... source on another GPU, no peer access: hipMemcpyPeerAsync into a staging strip, then added
 *   IPC_LOCAL     polaris_hip_merge_ipc, the peer's ring lives on dst's own GPU
 *   IPC_PEER      polaris_hip_merge_ipc, the peer's ring lives on another GPU and is read directly
 *   IPC_UNKNOWN   no longer counted: a ring of unknown whereabouts (no bus id on either side) was read directly; it now goes through
 *                 the staging strip and counts as IPC_STAGED (the constant stays: ABI)
 *   IPC_STAGED    polaris_hip_merge_ipc, the ring is not KNOWN to be reachable (hipDeviceCanAccessPeer = 0 or failed, no bus id): the rows are
 *                 copied into a staging strip by the runtime (hipMemcpyAsync, which may go through the host) and added from there --
 *                 a kernel is never pointed at memory the device cannot reach
 *   DEVICE_STRIP  polaris_hip_merge_device (a strip some transport delivered: bench.py's fallback)
 * bench.py reports them in config.exchange_detail: a fallback that ran silently shows in the numbers' own line. */
#define POLARIS_MERGE_LOCAL 0
#define POLARIS_MERGE_PEER_ACCESS 1
#define POLARIS_MERGE_STAGED 2
#define POLARIS_MERGE_IPC_LOCAL 3
#define POLARIS_MERGE_IPC_PEER 4
#define POLARIS_MERGE_IPC_UNKNOWN 5
#define POLARIS_MERGE_DEVICE_STRIP 6
#define POLARIS_MERGE_IPC_STAGED 7
#define POLARIS_MERGE_BRANCHES 8
int polaris_hip_merge_counts(polaris_hip_tracer *dst, uint64_t counts[POLARIS_MERGE_BRANCHES]);

/* The pipeline's Reset stage on its own (tracer/opencl/tracer.go:208-213: clearAccumulator(frameAccumulator)).
 * Trace runs it whenever accumulated_samples == 0.  A host that merges a frame's blocks only after the NEXT
 * frame's Trace has started (bench.py keeps the strip exchange one frame behind the tracing) calls it before
 * merging, so that exactly one frame's blocks are ever summed.  Asynchronous on the handle's stream. */
int polaris_hip_reset_frame(polaris_hip_tracer *h);

/* Ordering merges from other threads against the Reset stage without waiting for a whole Trace.  The reset epoch of a
 * tracer counts the Traces with accumulated_samples == 0 (and reset_frame calls) that have queued the clear of the frame
 * accumulator -- or have failed before they could.  A frame loop reads the primary's epoch before it hands out the
 * frame's blocks; a worker that is about to merge into the primary first waits for the epoch to pass that value: its
 * merge then lands behind this frame's clear, while the primary is still tracing (the reference leaves this to chance,
 * renderer/default.go:188-191 against tracer.go:208-213; polaris_amd/host/renderer.cpp shows the use). */
int polaris_hip_reset_epoch(polaris_hip_tracer *h, uint64_t *epoch);
int polaris_hip_wait_reset(polaris_hip_tracer *h, uint64_t epoch); /* POLARIS_E_TIMEOUT after 120 s without that Reset */

/* Tracer.SyncFramebuffer: wait for pending merges, then tonemapSimpleReinhard over rows of
 * req with weight 1/(accumulated_samples+samples_per_pixel) into the RGBA8 frame buffer.
 * With denoising on (polaris_hip_set_denoise, iterations > 0) the rows of req are first filtered into the DENOISED plane
 * (edge-avoiding a-trous wavelet filter over the running mean, guided by the first-hit G-buffer, which is computed at the first
 * denoised sync after a resize / upload_scene / set_camera), and that plane is tone-mapped with weight 1 instead.  The
 * accumulators are never written by the filter; rows outside req keep their frame buffer bytes.  Denoising needs a camera. */
int polaris_hip_sync_framebuffer(polaris_hip_tracer *h, const PolarisBlockRequest *req);

/* Denoising of the synced frame (no reference counterpart: the reference's SyncFramebuffer only tone-maps; "run post-process
 * filters to the accumulated trace data", tracer/tracer.go:108-110).  Off by default; with it off sync_framebuffer allocates and
 * launches nothing new.  Per pixel i of the request's rows, with c = frame accumulator rgb * weight, the G-buffer's shading normal n
 * and hit distance t, and the first hit's albedo a:  r0 = c / max(a, 1e-3); K iterations k of a 5 x 5 B3-spline kernel at stride
 * 2^k whose taps j are weighted by max(0, n_i . n_j)^(2^P) * exp(-|t_i - t_j| / (sigma_depth * 2^k * t_i))
 * * exp(-|m(r_i) - m(r_j)|^2 / (sigma_luminance^2 * 2^-k)), m(x) = x / (x + 1); result r_K * max(a, 1e-3).  Misses and emitters
 * pass through and are never taps; taps outside the request's rows are skipped.  DESIGN.md 10 has the exact arithmetic.
 * Suggested settings (chosen on the CPU restatement): iterations 4, normal_power_log2 5, sigma_depth 0.1,
 * sigma_luminance 4.0.  A field out of range is POLARIS_E_BAD_ARGUMENT: iterations 0..8 (0 = off, the default),
 * normal_power_log2 0..10, sigmas 0 (term off) or within [1e-6, 1e6].  Set struct_size = sizeof(PolarisDenoiseParams). */
typedef struct PolarisDenoiseParams {
	uint32_t struct_size;        /* sizeof(PolarisDenoiseParams), as PolarisBvhBuildInput does */
	uint32_t iterations;         /* K: 0 = off (default), 1..8 */
	uint32_t normal_power_log2;  /* P: 0..10 */
	float    sigma_depth;        /* >= 0, finite; 0 = term off */
	float    sigma_luminance;    /* >= 0, finite; 0 = term off */
} PolarisDenoiseParams;
int polaris_hip_set_denoise(polaris_hip_tracer *h, const PolarisDenoiseParams *p);

/* Frame-sized float4 planes of the denoiser (n_floats >= frame_w*frame_h*4, row-major):
 *   GUIDE     first-hit shading normal xyz (after bump / normal maps) | hit distance; miss: 0, 0, 0, FLT_MAX
 *   ALBEDO    first-hit albedo rgb (clamp(tint * k, 0, 1) for diffuse / conductor / rough conductor leaves, 1 otherwise) | the
 *             selected leaf's type as int bits; miss: 1, 1, 1 | -1
 *   DENOISED  the filtered running mean of the last denoised sync (rows outside its request: whatever an earlier sync left)
 * With the option "guide_specular" = N > 0 "first hit" reads "the first surface the guide ray does not follow through" (at most N
 * mirror / glass links):
 *   GUIDE     that surface's shading normal | T, the float sum of the links' hit distances in order -- the unfolded path length:
 *             eye + T d is the mirror image of the surface for a chain of planar mirrors, an approximation through curved
 *             mirrors and refraction; a miss at any link is the miss above
 *   ALBEDO    the product of the followed links' albedo (the rule above at each: tint * k for a mirror, 1 for glass) and that
 *             surface's | that surface's leaf type.  An emitter seen in a mirror has type EMISSIVE: it passes through the filter
 *             and is never a tap
 * The G-buffer is ONE ray per pixel through the pixel centre, computed on first use and kept until resize / upload_scene /
 * set_camera / a change of "guide_specular".  GUIDE / ALBEDO: POLARIS_E_NO_SCENE_DATA without a scene, POLARIS_E_BAD_ARGUMENT without a camera; DENOISED:
 * POLARIS_E_BAD_ARGUMENT before any denoised sync. */
#define POLARIS_AOV_GUIDE    0
#define POLARIS_AOV_ALBEDO   1
#define POLARIS_AOV_DENOISED 2
/*   TEMPORAL  the running mean blended with the history of the last temporal sync (rgb | effective sample count n + m)
 *   PRIOR     the history reprojected into the current camera (rgb h | m, m = 0: no history)
 * TEMPORAL / PRIOR: POLARIS_E_BAD_ARGUMENT before any temporal sync (polaris_hip_set_temporal) under the current camera. */
#define POLARIS_AOV_TEMPORAL 3
#define POLARIS_AOV_PRIOR    4
/*   VARIANCE  M1 | M2 | n_eff | v: the luminance of the synced mean, the mean of L^2, the effective sample count and the variance
 *             of the mean (polaris_hip_set_variance); v = 0 for misses and emitters
 *   PRIOR2    with temporal reuse as well: the history's M2 reprojected into the current camera (h2 | 0 | 0 | m)
 * VARIANCE / PRIOR2: POLARIS_E_BAD_ARGUMENT before any variance sync (under the current camera with temporal reuse). */
#define POLARIS_AOV_VARIANCE 5
#define POLARIS_AOV_PRIOR2   6
int polaris_hip_read_aov(polaris_hip_tracer *h, int which, float *out, size_t n_floats);

/* Temporal reuse of the synced frame across camera moves (no reference counterpart: the reference's interactive renderer resets
 * its accumulation on every move, renderer/opengl.go:294-301).  Off by default (max_history = 0); with it off sync_framebuffer,
 * set_camera, resize and upload_scene allocate and launch nothing new.  With it on the tracer keeps a HISTORY: the TEMPORAL plane,
 * G-buffer and camera of the last temporal sync before the latest set_camera (pointer swaps, no copies).  At the first temporal
 * sync under a camera the history is reprojected into the PRIOR: for every filtered pixel i (a first hit that is not an emitter)
 * p = eye + t_i d_i is projected into the history camera, and of the 2 x 2 history pixels around it those with a count > 0,
 * finite rgb, pixel i's leaf type, n_i . n_j >= normal_threshold and |t_j - |p - eye'|| <= depth_threshold |p - eye'| are
 * blended bilinearly (weights renormalised): h, m = min(count, max_history).  Every temporal sync then writes the request's rows of
 * TEMPORAL = (acc + m h) / (n + m) where m > 0 and acc / n (sync's expression, bit for bit) where m = 0, n = accumulated_samples +
 * samples_per_pixel, and the denoiser (if on) or the tone-map runs on TEMPORAL with weight 1.  The accumulators are never
 * written.  A history camera whose frustum corners are not a parallelogram (some w != 0, or |tl + br - tr - bl| >
 * 1e-3 |tr - tl|) gives no history.  Resize, upload_scene and max_history = 0 drop the history.  DESIGN.md 10b has the exact
 * arithmetic.  Suggested settings (chosen on the CPU restatement): max_history 32, normal_threshold 0.9,
 * depth_threshold 0.1.  A field out of range is POLARIS_E_BAD_ARGUMENT: max_history 0..4096, normal_threshold within [-1, 1],
 * depth_threshold within [0, 1e6].  Set struct_size = sizeof(PolarisTemporalParams). */
typedef struct PolarisTemporalParams {
	uint32_t struct_size;       /* sizeof(PolarisTemporalParams) */
	uint32_t max_history;       /* cap on the history's sample count m: 0 = off (default), 1..4096 */
	float    normal_threshold;  /* a history tap needs n_i . n_j >= this */
	float    depth_threshold;   /* ... and |t_j - d| <= this * d, d = the point's distance from the history eye */
} PolarisTemporalParams;
int polaris_hip_set_temporal(polaris_hip_tracer *h, const PolarisTemporalParams *p);

/* Variance-guided denoising (SVGF, Schied et al. 2017; no reference counterpart).  Off by default (sigma_variance = 0); with it off
 * every sync runs and allocates exactly what it did.  Needs the option "moments" = 1 on this tracer first (else
 * POLARIS_E_BAD_ARGUMENT).  With it on, every sync writes the request's rows of the VARIANCE plane from the frame accumulator
 * (rgb | sum L^2), n = accumulated_samples + samples_per_pixel: M1 = lum(mean), M2 = sum L^2 / n (with temporal reuse and a history
 * m > 0: (sum L^2 + m h2) / (n + m), n_eff = n + m), and for every filtered pixel v = max(0, M2 - M1^2) / (n_eff - 1) where
 * n_eff >= max(min_samples, 2), else a 7 x 7 spatial estimate weighted by the denoiser's normal and depth terms, divided by n_eff.
 * With denoise iterations > 0 the a-trous filter's luminance term becomes exp(-|lum(r_i) - lum(r_j)| / (sigma_variance
 * sqrt(g3x3(v_i)) + 1e-10)) and the variance is filtered alongside (w^2 v / (sum w)^2); the DENOISED plane's .w holds it.  With
 * iterations = 0 the frame-buffer bytes are those of the plain sync.  DESIGN.md 10c has the exact arithmetic and the suggested
 * settings (polaris_amd/ctypes_api.py VARIANCE_DEFAULTS).  A field out of range is POLARIS_E_BAD_ARGUMENT: sigma_variance 0 or
 * within [1e-6, 1e6], min_samples 1..64 (not looked at while off).  Set struct_size = sizeof(PolarisVarianceParams). */
typedef struct PolarisVarianceParams {
	uint32_t struct_size;       /* sizeof(PolarisVarianceParams) */
	float    sigma_variance;    /* sigma_v of the luminance term: 0 = off (default) */
	uint32_t min_samples;       /* pixels with fewer effective samples take the spatial estimate */
} PolarisVarianceParams;
int polaris_hip_set_variance(polaris_hip_tracer *h, const PolarisVarianceParams *p);

/* The display transform of polaris_hip_sync_framebuffer (no reference counterpart: the reference's is tonemapSimpleReinhard with the
 * request's exposure and pow(1 / 2.2)).  Off by default (enabled = 0); with it off every sync runs and allocates exactly what it did,
 * under the same kernel symbols.  With it on the sync's last step -- k_tonemap of the frame accumulator with the sync's weight, or of
 * the TEMPORAL / DENOISED plane with weight 1 -- is replaced, over the request's rows, by
 *   auto_exposure = 1:  k_meter   a 256-bin histogram of L = lum(rgb * weight) (Rec. 709, without the request's exposure) of the
 *                                 pixels whose L is finite and >= 2^-16: 8 bins an octave over [2^-16, 2^16) taken from the float's
 *                                 exponent and top three mantissa bits, L >= 2^16 in bin 255; integer atomics, exact in any schedule;
 *                       k_expose  N = the metered count; the window is the pixels of rank [N low_permille / 1000,
 *                                 max(N high_permille / 1000, that + 1)) in ascending bins (64-bit integers); avg = the window's mean of
 *                                 the bins' log2 values e + log2(1 + (k + 1/2) / 8); target = clamp(log2(key) - avg + compensation_ev,
 *                                 min_ev, max_ev); log2E = target at the first metered sync after a reset, else
 *                                 log2E + (target - log2E) * adapt; E = exp2(log2E).  N = 0 (a black or all-NaN frame): the state
 *                                 stays, E = exp2(log2E) with a state and 1 without;
 *   always:             k_display per channel c = rgb * weight * request.exposure * E (E = 1 with auto_exposure = 0), the tone operator,
 *                                 the transfer function, clamp to [0, 1], times 255, truncated.
 * Everything runs on the device inside the sync: the exposure a sync meters is the exposure it displays with.  The exposure state
 * (log2E and whether it is set) is reset by polaris_hip_resize and by a polaris_hip_set_display that changes a byte of the params; it
 * survives set_camera, upload_scene and the in-place updates.  Metering looks at the rows of the request on this tracer only.
 * REINHARD with srgb = 0 and auto_exposure = 0 gives k_tonemap's bytes bit for bit.  DESIGN.md 10l has the exact arithmetic.
 * Tone operators, c -> m:  REINHARD c / (c + 1);  REINHARD_WHITE c (1 + c / white^2) / (1 + c);  ACES (Narkowicz's fit)
 * c (2.51 c + 0.03) / (c (2.43 c + 0.59) + 0.14);  HABLE f(c) / f(white), f(x) = (x (0.15 x + 0.05) + 0.004) / (x (0.15 x + 0.5) + 0.06)
 * - 0.02 / 0.3.  Transfer, m -> [0, 1]:  srgb = 0 pow(m, 1 / 2.2);  srgb = 1 the sRGB OETF, 12.92 m up to 0.0031308, else
 * 1.055 pow(m, 1 / 2.4) - 0.055.
 * A field out of range is POLARIS_E_BAD_ARGUMENT and leaves the state unchanged: enabled, srgb, auto_exposure 0 or 1; tone_operator
 * 0..3; white within [1e-3, 1e6] (looked at by REINHARD_WHITE and HABLE, checked always); with auto_exposure = 1 also key within
 * [1e-6, 1e6], compensation_ev, min_ev and max_ev within [-24, 24] with min_ev <= max_ev, low_permille < high_permille <= 1000 and
 * adapt within (0, 1].  With enabled = 0 no other field is looked at and any two off states are equal; with auto_exposure = 0 the
 * metering fields are not looked at.  A call with identical bytes does nothing.  polaris_amd/ctypes_api.py DISPLAY_DEFAULTS has the
 * suggested settings.  Set struct_size = sizeof(PolarisDisplayParams). */
#define POLARIS_TONE_REINHARD       0
#define POLARIS_TONE_REINHARD_WHITE 1
#define POLARIS_TONE_ACES           2
#define POLARIS_TONE_HABLE          3
typedef struct PolarisDisplayParams {
	uint32_t struct_size;       /* sizeof(PolarisDisplayParams) */
	uint32_t enabled;           /* 0 = off (default): the sync ends with k_tonemap */
	uint32_t tone_operator;     /* POLARIS_TONE_* */
	uint32_t srgb;              /* 0: pow(1 / 2.2), 1: the sRGB OETF */
	float    white;             /* the radiance mapped to 1 by REINHARD_WHITE and HABLE */
	uint32_t auto_exposure;     /* 1: meter the frame and multiply by the metered exposure E */
	float    key;               /* the luminance the metered window's log-average is mapped to (0.18: middle grey) */
	float    compensation_ev;   /* added to the target log2 exposure */
	uint32_t low_permille;      /* the metered window: the pixels between these two quantiles of luminance */
	uint32_t high_permille;
	float    min_ev, max_ev;    /* the target log2 exposure is clamped to [min_ev, max_ev] */
	float    adapt;             /* the fraction of the way to the target one sync moves (1: snap) */
} PolarisDisplayParams;
int polaris_hip_set_display(polaris_hip_tracer *h, const PolarisDisplayParams *p);

/* What the last sync with auto-exposure on metered: n_metered pixels, the window's mean log2 luminance avg, the state's log2E after
 * the sync and the exposure E it displayed with; valid = 0: nothing has been metered since the last reset (E = 1).  histogram (may be
 * NULL): the 256 counts of that sync.  POLARIS_E_BAD_ARGUMENT before any such sync since the last reset of the exposure state, or
 * with out null or another struct_size. */
typedef struct PolarisExposureInfo {
	uint32_t struct_size;       /* sizeof(PolarisExposureInfo) */
	uint32_t valid;
	uint64_t n_metered;
	float    avg, log2E, E;
	uint32_t reserved;
} PolarisExposureInfo;
int polaris_hip_read_exposure(polaris_hip_tracer *h, PolarisExposureInfo *out, uint32_t histogram[256]);

/* Bloom: a glare term of the display stage (no reference counterpart).  Off by default (enabled = 0), and in effect only while the display
 * stage is enabled (polaris_hip_set_display): a set_bloom with the display off is accepted, stored, and takes effect when the display is
 * turned on.  While it is off or not in effect every sync runs and allocates exactly what it did, under the same kernel symbols.
 * In effect, between k_expose and the display step, over the request's rows [y0, y1) alone (rows outside are never read; every
 * coordinate is clamped to its level's extent), everything in float32 in the order written:
 *   levels      w_0 = W, h_0 = y1 - y0; w_l = (w_{l-1} + 1) / 2, h_l = (h_{l-1} + 1) / 2; L = min(levels, the first l with w_l = h_l = 1);
 *   bright pass per source pixel and channel c = rgb * weight * exposure * E (the display step's value); NaN or <= 0 becomes 0, above 65536
 *               becomes 65536; m = max(r, g, b), k = threshold * knee, s = clamp(m - threshold + k, 0, 2 k), s = s s / (4 k + 1e-5);
 *               b = c * (max(s, m - threshold) / max(m, 1e-5));
 *   down        D_l(x, y) = sum over j = 0..3 of K[j] * (sum over i = 0..3 of K[i] * src(2 x - 1 + i, 2 y - 1 + j)), K = {1, 3, 3, 1} / 8,
 *               src = b for l = 1 (fused: the bright pass has no plane) and D_{l-1} above; karis = 1, level 1 only: every tap is
 *               weighted by 1 / (1 + luminance(b)) and the sum divided by the same sum of the weights (firefly suppression);
 *   up          U_L = D_L; U_l = D_l + up(U_{l+1}), in place; up is the 2 x tent: fine index i takes coarse (i >> 1) - 1 and i >> 1 with
 *               weights 1/4, 3/4 (even i), i >> 1 and (i >> 1) + 1 with 3/4, 1/4 (odd i), x inside y;
 *   display     k_display_bloom<OP, SRGB>: c + intensity * (up(U_1)(x, y) / L) per channel through the tone operator and the transfer
 *               function of PolarisDisplayParams (no full-resolution bloom plane exists).
 * The accumulators and counters are never touched.  The pyramid (sum of w_l h_l float4, about a third of a frame) is allocated by the first
 * bloomed sync and freed when bloom or the display goes off and by polaris_hip_resize.  A call with identical bytes does nothing; a changed
 * call touches only the pyramid: the exposure state, the temporal history and the G-buffer stay.  POLARIS_E_BAD_ARGUMENT with the state
 * unchanged: enabled or karis > 1; with enabled = 1 levels outside 1..8, or a float that is not finite or outside threshold [0, 65536],
 * knee [0, 1], intensity [0, 16].  With enabled = 0 nothing after it but karis is looked at and any two off states are equal.  The option
 * "bloom_fused" (default 0: one launch per level) set to 1 runs the levels of at most 1024 pixels in one launch (k_bloom_tail); the values
 * are the same bit for bit.  polaris_amd/ctypes_api.py BLOOM_DEFAULTS has the suggested settings.  DESIGN.md 10m. */
typedef struct PolarisBloomParams {
	uint32_t struct_size;  /* sizeof(PolarisBloomParams) */
	uint32_t enabled;      /* 0 = off (default) */
	uint32_t levels;       /* 1..8 pyramid levels asked for; fewer are used where the region runs out */
	float    threshold;    /* the displayed-linear value (after weight, exposure and E) above which a pixel blooms */
	float    knee;         /* 0..1: soft-knee fraction of threshold */
	float    intensity;    /* 0..16: factor of the bloom term added before the tone operator */
	uint32_t karis;        /* 0 / 1: weight the first downsample by 1 / (1 + luminance) */
} PolarisBloomParams;
int polaris_hip_set_bloom(polaris_hip_tracer *h, const PolarisBloomParams *p);

/* frame_w*frame_h*4 bytes RGBA8 (pipeline.go:226-232). */
int polaris_hip_read_framebuffer(polaris_hip_tracer *h, uint8_t *rgba, size_t n_bytes);

/* Radiance-level read-back for parity tests (no reference counterpart): which = 0 trace
 * accumulator, 1 frame accumulator; n_floats = frame_w*frame_h*4 (float3 at stride 4).  The .w of every pixel is the sum of the
 * samples' squared luminance with the option "moments" on, and 0 otherwise. */
int polaris_hip_read_accumulator(polaris_hip_tracer *h, int which, float *out, size_t n_floats);

/* Test tap: generate + intersect the primary rays of one sample with camera seed `seed` and
 * return rays [N][8], hit flags [N], (w,u,v,t) [N][4] and (instance, triangle) [N][2];
 * N = frame_w*block_h.  Any output pointer may be NULL.  With the lens on (polaris_hip_set_lens) the rays are k_generate_lens':
 * rays[i][0..2] is ray i's own origin on the lens; with the shutter on (polaris_hip_set_shutter) they are k_generate_shutter's. */
int polaris_hip_tap_primary(polaris_hip_tracer *h, const PolarisBlockRequest *req, uint32_t seed,
                            float *rays, int32_t *hit, float *wuvt, int32_t *tri);

/* Function-level test taps: the device-side samplers and BxDFs of the uploaded scene on caller-supplied
 * inputs, one probe per row of `in`, through the same table staging the shade kernels use.
 *   kind 0, BxDF of material LEAF node `index` (bxdf/bxdf.cl:31-105):
 *        in [n][13] = normal[3] uv[2] in_dir[3] sample[2] eval_dir[3]
 *        out[n][11] = bxdfGetSample value[3], sampled dir[3], pdf | bxdfGetPdf(eval_dir) | bxdfEval(eval_dir)[3]
 *   kind 1, texture `index` (samplers/texture_sampler.cl:14-252):
 *        in [n][2] = uv;  out[n][7] = texGetSample3f[3] | texGetSample1f | texGetBumpSample3f[3]
 *   kind 2, emissive `index` (samplers/emissive_sampler.cl:176-223):
 *        in [n][11] = point[3] normal[3] sample[2] pdf_dir[3]
 *        out[n][9]  = emissiveGetSample radiance[3] dir[3] pdf dist | emissiveGetPdf(pdf_dir)
 *   kind 3, material tree rooted at node `index` (matSelectNode, samplers/material_sampler.cl:21-95):
 *        in [n][8]  = normal[3] uv[2] | shading PRNG state[2] and path dispersion flags as bit patterns
 *        out[n][18] = selected leaf type (bits), int / ext IOR after the dispersion override | normal after bump / normal
 *                     maps[3] | tint[3] | path flags (bits) | PRNG state[2] (bits) | the leaf's k[3] and t[3] */
int polaris_hip_probe(polaris_hip_tracer *h, int kind, uint32_t index, uint32_t n, const float *in, float *out);

/* rayIntersectionQuery (any_hit = 0, kernels/intersect.cl:184-347) or rayIntersectionTest (any_hit != 0, :26-180) over n
 * arbitrary rays [n][8] = origin.xyz, maxDist, dir.xyz, unused, through the traversal kernel the options select
 * ("traversal", "node_mode", "packet_primary" = 1 / "packet_shadow" > 0 for the wave-packet kernel): hit[n]; for closest
 * hits also (w,u,v,t) [n][4] and the scene triangle index [n] (-1 = miss); either may be NULL. */
int polaris_hip_probe_intersect(polaris_hip_tracer *h, const float *rays, uint32_t n, int any_hit, int32_t *hit,
                                float *wuvt, int32_t *tri);

/* Self-test of the one place where the kernels do NOT use the compiler's correctly rounded division: 1 / det of the
 * triangle tests is v_rcp_f32 + one Newton step (3 instructions instead of 11).  Sweeps all 2^32 float bit patterns x on the
 * device and counts those whose result differs from 1.0f / x, inside and outside lo <= |x| <= hi (`sample` = one differing
 * pattern inside, may be NULL).  The claim the kernels rest on: none inside [2^-126, 2^126).  (The directions in
 * polaris_hip_probe_intersect must be finite with components <= 2^10, origins <= 2^40; scenes: DESIGN.md 2.) */
int polaris_hip_selftest_rcp(polaris_hip_tracer *h, float lo, float hi, uint64_t *mismatches_inside, uint64_t *mismatches_outside,
                             uint32_t *sample);

/* Self-test of include/polaris_math.h as this library's build compiled it (polaris_amd/csrc/builtin_probe.h): inputs
 * [first, first + count) of built-in fn (PbFn: unary functions over all 2^32 bit patterns, binary / ternary ones over an edge
 * grid and 2^28 counter-based draws) evaluated on the device.  fingerprints (may be NULL; first a multiple of 2^20): per chunk
 * c of 2^20 inputs from first, [2c] = the fingerprint of its inputs inside fn's domain, [2c + 1] outside.  results (may be
 * NULL; count <= 2^POLARIS_SELFTEST_MAX_RESULTS_LOG2): the result bits per input.  The CPU oracle computes the same
 * (polaris_oracle_builtins), so every chunk must agree (tests/test_gpu_builtins_device.py). */
#define POLARIS_SELFTEST_MAX_RESULTS_LOG2 24
int polaris_hip_selftest_builtins(polaris_hip_tracer *h, uint32_t fn, uint64_t first, uint64_t count, uint64_t *fingerprints,
                                  uint32_t *results);

/* Test entry of the denoiser's filter on caller planes: acc, guide, albedo are W x H float4 planes as the frame accumulator and
 * the G-buffer (POLARIS_AOV_GUIDE / _ALBEDO); rows [block_y, block_y + block_h) are filtered with *p (iterations >= 1) and
 * weight into denoised, then tone-mapped with weight 1 and exposure into rgba (W x H x 4 bytes) -- the launches of a denoised
 * polaris_hip_sync_framebuffer.  denoised and rgba are in / out: their other rows come back as given.  Uses buffers of its
 * own; no state of the tracer is read or changed. */
int polaris_hip_denoise_planes(polaris_hip_tracer *h, const float *acc, const float *guide, const float *albedo, uint32_t W, uint32_t H,
                               uint32_t block_y, uint32_t block_h, float weight, float exposure, const PolarisDenoiseParams *p,
                               float *denoised, uint8_t *rgba);

/* Test entry of variance guidance on caller planes: acc (rgb | sum L^2, `samples` samples a pixel), guide and albedo are W x H float4
 * planes; k_variance over the rows [block_y, block_y + block_h) into `variance`, then (p->iterations > 0) the variance-guided filter
 * into `denoised` and its tone-map into rgba, or (iterations = 0) the plain tone-map of acc / samples -- the launches of a variance
 * sync without temporal reuse.  The rows outside the request keep the bytes the caller passed in.  sigma_variance must be non-zero. */
int polaris_hip_variance_planes(polaris_hip_tracer *h, const float *acc, const float *guide, const float *albedo, uint32_t W, uint32_t H,
                                uint32_t block_y, uint32_t block_h, uint32_t samples, float exposure, const PolarisDenoiseParams *p,
                                const PolarisVarianceParams *v, float *variance, float *denoised, uint8_t *rgba);

/* Test entry of the display stage on a caller plane: plane is a W x H float4 plane (rgb | unused); the rows [block_y, block_y + block_h)
 * are metered (p->auto_exposure) with weight, exposed and displayed with weight and exposure into rgba (W x H x 4 bytes) -- the
 * launches k_meter, k_expose, k_display of a displayed polaris_hip_sync_framebuffer.  prev_log2E (may be NULL): the exposure state the
 * sync starts from, as left by an earlier metered sync; NULL: none, as after a reset.  rgba is in / out: its other rows come back as
 * given.  histogram (256 counts; may be NULL) and info (may be NULL; its struct_size set) are what polaris_hip_read_exposure would
 * return after the sync; with auto_exposure = 0 the counts are 0 and info is valid = 0, E = 1.  p->enabled must be 1.  Uses buffers
 * of its own; no state of the tracer is read or changed. */
int polaris_hip_display_planes(polaris_hip_tracer *h, const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h,
                               float weight, float exposure, const PolarisDisplayParams *p, const float *prev_log2E, uint8_t *rgba,
                               uint32_t histogram[256], PolarisExposureInfo *info);

/* Test entry of a bloomed displayed sync on a caller plane, as polaris_hip_display_planes: the rows [block_y, block_y + block_h) of plane
 * are metered (dp->auto_exposure), exposed from prev_log2E (may be NULL), bloomed (bp) and displayed into rgba (in / out: its other rows
 * come back as given) -- the launches k_meter, k_expose, the pyramid's and k_display_bloom of such a sync, with the tracer's option
 * "bloom_fused".  level1 (may be NULL): U_1, h_1 x w_1 x 4 floats; levels_used (may be NULL): L.  dp->enabled and bp->enabled must be 1.
 * Uses buffers of its own; no state of the tracer is read or changed. */
int polaris_hip_bloom_planes(polaris_hip_tracer *h, const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight,
                             float exposure, const PolarisDisplayParams *dp, const PolarisBloomParams *bp, const float *prev_log2E, uint8_t *rgba,
                             float *level1, uint32_t *levels_used);

/* Test entry of the temporal reprojection on caller planes: history (rgb | count), prev_guide, prev_albedo seen under the camera
 * (prev_eye, prev_frustum), and the current guide, albedo under (eye, frustum), all W x H float4 planes; the PRIOR plane of every
 * pixel into prior -- the launch of the first temporal sync after a set_camera.  Uses buffers of its own; no state of the tracer
 * is read or changed. */
int polaris_hip_reproject_planes(polaris_hip_tracer *h, const float *history, const float *prev_guide, const float *prev_albedo,
                                 const float prev_eye[3], const float prev_frustum[16], const float *guide, const float *albedo,
                                 const float eye[3], const float frustum[16], uint32_t W, uint32_t H, const PolarisTemporalParams *p,
                                 float *prior);

/* polaris_hip_reproject_planes with object motion (option "object_motion"): also the two INSTANCE planes (W x H words as
 * polaris_hip_read_instance_plane returns them; a word >= n_instances gives its pixel no history), the inv_transform tables of the
 * n_instances (1..2^20) mesh instances the history and the current frame were seen with (16 floats each, column major, as
 * PolarisMeshInstance) and, optionally, the history's VARIANCE plane with PRIOR2 as its output (both NULL or neither) -- the launch
 * of the first temporal sync after an upload_scene that moved instances.  Uses buffers of its own; no state of the tracer is read or
 * changed. */
int polaris_hip_reproject_motion_planes(polaris_hip_tracer *h, const float *history, const float *prev_guide, const float *prev_albedo,
                                        const uint32_t *prev_instance, const float prev_eye[3], const float prev_frustum[16], const float *guide,
                                        const float *albedo, const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t W,
                                        uint32_t H, uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                        const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2);

/* The INSTANCE plane of the first-hit G-buffer (option "object_motion"): per pixel the mesh-instance index of the hit POLARIS_AOV_GUIDE
 * describes, 0xFFFFFFFF for a miss (where GUIDE's t is FLT_MAX); n >= frame_w * frame_h words.  With the option "guide_specular" a
 * pixel whose guide ray followed at least one link is 0xFFFFFFFF too: the reprojection gives a word >= n_instances no history, so with
 * "object_motion" in effect what is seen through a mirror or glass takes none (with it off, camera moves reuse it).  Errors as polaris_hip_read_aov of
 * POLARIS_AOV_GUIDE; POLARIS_E_BAD_ARGUMENT with the option off, or without effect because temporal reuse is off. */
int polaris_hip_read_instance_plane(polaris_hip_tracer *h, uint32_t *out, size_t n);

/* polaris_hip_reproject_motion_planes with vertex motion (option "vertex_motion"): also the current frame's HIT plane (W x H x 4
 * words as polaris_hip_read_hit_plane returns them) and the vertices of the num_triangles (1..2^24) scene triangles as the scene holds
 * them now and as the history saw them ([3 num_triangles][4] floats each, scene order, w ignored).  A pixel whose HIT triangle is
 * >= num_triangles or whose INSTANCE word is >= n_instances has no history; one whose triangle has the same 36 bytes of xyz in both
 * arrays is reprojected as by polaris_hip_reproject_motion_planes; any other from the point of the old triangle at the hit's
 * barycentrics, taken to the world through inverse(prev_inv_transforms[k]) -- the launch of the first temporal sync after an
 * update_vertices.  Uses buffers of its own; no state of the tracer is read or changed. */
int polaris_hip_reproject_deform_planes(polaris_hip_tracer *h, const float *history, const float *prev_guide, const float *prev_albedo,
                                        const uint32_t *prev_instance, const float prev_eye[3], const float prev_frustum[16], const float *guide,
                                        const float *albedo, const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t W,
                                        uint32_t H, uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                        const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2,
                                        const uint32_t *hit, const float *vertices, const float *prev_vertices, uint32_t num_triangles);

/* The HIT plane of the first-hit G-buffer (option "vertex_motion"): per pixel four words, the scene triangle of the hit
 * POLARIS_AOV_GUIDE describes | the bits of its barycentric u | of v | 0 -- what the surface was interpolated from; 0xFFFFFFFF | 0 |
 * 0 | 0 for a miss and, with the option "guide_specular", for a pixel whose guide ray followed at least one link (as the INSTANCE
 * word).  n_words >= 4 * frame_w * frame_h.  Errors as polaris_hip_read_instance_plane; POLARIS_E_BAD_ARGUMENT with the option off or
 * not in effect. */
int polaris_hip_read_hit_plane(polaris_hip_tracer *h, uint32_t *out, size_t n_words);

/*
 * Move mesh instances in place (no reference counterpart: the reference uploads the whole scene, tracer.go:166-173).
 * Synchronous, under the handle's mutex, behind every stream of the handle, like an upload.  Afterwards the tracer behaves bit for
 * bit as if polaris_hip_upload_scene had been given the uploaded scene's arrays with three substitutions:
 *   - mesh_instances[i].inv_transform = inv_transforms[i];
 *   - emissives = the new list (NULL: unchanged).  Only `transform` and `area` of an entry may differ from the uploaded list;
 *   - the top-level BVH nodes REFIT: a top-level leaf takes instance_boxes[i] verbatim (also a box that does not bound its
 *     instance: the scene reader's translation-only boxes survive), a top-level inner node the component-wise minimum / maximum of
 *     its two children (fmin / fmax of finite values; where +0 meets -0, the left child's).
 * Topology, child order, mesh trees, triangle records and everything else stay as uploaded.  The library recomputes what a full
 * upload derives from these: the Inst records, the boxes and cull factors of the top-level pair records (the exact world extent
 * of every instance's mesh, on the device), the padding of the boxes leaf subdivision added (it depends on the matrices and the
 * world box: every update RE-PADS those boxes, and no move is refused for the padding's sake), the light geometry derived from
 * `transform` and `area`.
 * One deviation: build_layout bounds an instance by the eight corners of its mesh's box once a scene needs more than 32 M / 3
 * vertex transforms, the update always by all vertices, so above that cap a cull factor may be 1.001 where a full upload has
 * +inf -- only ever where culling is legal; results are the same.
 * To the temporal history the call is what an upload_scene is: with "object_motion" in effect the planes synced under the old
 * matrices join the history and it is kept (instances and meshes are the same); without, the history is dropped.  The G-buffer is
 * invalidated.
 * A failing HIP call (POLARIS_E_DEVICE) after the arguments were accepted leaves the scene as a failed upload_scene does: upload again.
 * Refusals leave the tracer's state unchanged: POLARIS_E_NO_SCENE_DATA before an upload; POLARIS_E_UNSUPPORTED when the scene was
 * uploaded with "instance_update" off; POLARIS_E_BAD_ARGUMENT for a wrong struct_size, a wrong instance count, null pointers, or an
 * emissive list whose count or per-entry type / tri_index / mat_node_index differs from the uploaded one; POLARIS_E_BAD_SCENE for a
 * matrix entry not finite or beyond 2^30 (the upload's own rule) and for a box that is not finite or has min > max.
 */
typedef struct PolarisInstanceUpdate {
	uint32_t struct_size;             /* = sizeof(PolarisInstanceUpdate) */
	uint32_t num_mesh_instances;      /* must equal the uploaded scene's */
	const float *inv_transforms;      /* [NI][16], column major, as PolarisMeshInstance.inv_transform */
	const float *instance_boxes;      /* [NI][6] world-space min.xyz, max.xyz: the scene reader's boxes, as in PolarisBvhBuildInput */
	const PolarisEmissive *emissives; /* NULL = unchanged; else [num_emissives] */
	uint32_t num_emissives;
} PolarisInstanceUpdate;
int polaris_hip_update_instances(polaris_hip_tracer *h, const PolarisInstanceUpdate *u);

/* Deform the uploaded scene's meshes in place (no reference counterpart).  The scene must have been uploaded with the
 * option "vertex_update" on.  Synchronous, under the handle's mutex, behind every stream, like an upload.  Afterwards the tracer
 * behaves -- accumulators, counters, probes, taps, G-buffer planes -- bit for bit as a fresh tracer does after polaris_hip_upload_scene
 * of the uploaded scene's arrays with these substitutions:
 *   - vertices = the new ones; normals = the new ones (NULL: unchanged);
 *   - the mesh BVH nodes (every node below a mesh root, the root included) REFIT on the unchanged topology: a triangle leaf takes the
 *     exact bounds of its triangles' vertices, an inner node the union of its two children.  Minimum and maximum are b < a ? b : a
 *     and b > a ? b : a with a the running value, folded over the leaf's triangles in its own order, of each v0, v1, v2; for an inner
 *     node the left child before the right.  Where +0 meets -0 the earlier operand stays;
 *   - mesh_instances[i].inv_transform = inv_transforms[i] (NULL: unchanged);
 *   - the top-level nodes refit as polaris_hip_update_instances defines, from instance_boxes;
 *   - emissives = the new list (NULL: unchanged).  Only `transform` and `area` of an entry may differ from the uploaded one: the
 *     area of an area light changes when its triangle deforms, and the caller supplies it.
 * Two things do not follow the deformation, and neither can change a result.  The topology leaf subdivision ADDED below the caller's
 * leaves was chosen from the uploaded vertices and is kept; its boxes become the exact bounds of the triangles below them with the
 * padding a full upload would compute now, so they still only cull inside a leaf of the caller's tree (a full upload of the refit
 * scene may split its leaves differently: with max_leaf_tris != 0 the records are not comparable byte for byte, the results are).
 * And the slot order of a scene of at most 2 046 slots (it follows the leaf areas at upload) and the kernel selection (node mode,
 * tiny_one, packet use) stay as uploaded.
 * To the temporal history the call is a scene it never saw: the history is dropped, with "object_motion" on or off, and the G-buffer
 * is invalidated.
 * A failing HIP call (POLARIS_E_DEVICE) after the arguments were accepted leaves the scene as a failed upload_scene does: upload again.
 * Refusals are decided on the host before anything is touched and leave the tracer's state unchanged: POLARIS_E_NO_SCENE_DATA before
 * an upload; POLARIS_E_UNSUPPORTED when the scene was uploaded with "vertex_update" off, or when no mesh plan could be kept (two mesh
 * roots share a subtree: the message names the node); POLARIS_E_BAD_ARGUMENT for a wrong struct_size, wrong counts, null vertices or
 * instance_boxes, or an emissive list whose count or per-entry type / tri_index / mat_node_index differs from the uploaded one;
 * POLARIS_E_BAD_SCENE for a vertex coordinate not finite or beyond 2^40, a matrix entry not finite or beyond 2^30 (the upload's own
 * rules and texts) and for a box that is not finite or has min > max.
 */
typedef struct PolarisVertexUpdate {
	uint32_t struct_size;             /* = sizeof(PolarisVertexUpdate) */
	uint32_t num_triangles;           /* must equal the uploaded scene's */
	const float *vertices;            /* [3 NT][4], as PolarisSceneView.vertices */
	const float *normals;             /* NULL = unchanged; else [3 NT][4] */
	uint32_t num_mesh_instances;      /* must equal the uploaded scene's */
	const float *instance_boxes;      /* [NI][6]: the scene reader's world boxes for the deformed meshes */
	const float *inv_transforms;      /* NULL = unchanged; else [NI][16] column major */
	const PolarisEmissive *emissives; /* NULL = unchanged; else [num_emissives] */
	uint32_t num_emissives;
} PolarisVertexUpdate;
int polaris_hip_update_vertices(polaris_hip_tracer *h, const PolarisVertexUpdate *u);

/* Edit the uploaded scene's materials in place (no reference counterpart).  No upload option: every upload holds what
 * the call needs.  Synchronous, under the handle's mutex, behind every stream, like an upload.  Afterwards the tracer behaves --
 * accumulators, counters, probes, taps, G-buffer planes, the triangle records and the mask of emitting shading classes themselves --
 * bit for bit as a fresh tracer does after polaris_hip_upload_scene of the uploaded scene's arrays with these substitutions:
 *   - material_nodes = the new table (the same number of nodes: callers who want headroom upload spare, unreferenced leaves);
 *   - material_index = the new roots (NULL: unchanged);
 *   - scene_diffuse_mat_index = the given one (always taken: pass the uploaded value to keep it; -1 = no background);
 *   - emissives[e].mat_node_index = emissive_mat_nodes[e] (NULL: unchanged).  The emissive list keeps its count, triangles, types,
 *     transforms and areas: turning triangles into lights or removing lights needs an upload (a radiance of zero covers "off").
 * The library recomputes what a full upload derives from these: the shading class of every material node, the class in the two words
 * of every triangle record that carry it (kernel k_retag, timer "retag") and the mask of classes that can end in an emitter.
 * Geometry, trees, slot order, node mode and the kernel selection do not depend on materials and stay.  No semantic check is made
 * beyond the upload's own: an emissive entry whose triangle no longer has an emissive material behaves as after an upload of such arrays.
 * polaris_hip_update_texture replaces the texels of ONE texture, same format and size as uploaded: n_bytes must equal
 * bytes per texel * width * height of texture `index`.
 * To the temporal history both calls are a scene it never saw: the history is dropped, with "object_motion" on or off, and the
 * G-buffer is invalidated (the ALBEDO plane changes).
 * A failing HIP call (POLARIS_E_DEVICE) after the arguments were accepted leaves the scene as a failed upload_scene does: upload again.
 * Refusals are decided on the host before anything is touched and leave the tracer's state unchanged: POLARIS_E_NO_SCENE_DATA before
 * an upload; POLARIS_E_BAD_ARGUMENT for a wrong struct_size, null material_nodes, a node, triangle or emissive count that differs
 * from the uploaded one, a texture index out of range or an n_bytes that is not the texture's size; POLARIS_E_BAD_SCENE for every
 * material rule of the upload, with the upload's text (unknown operator, child / texture / transmittance texture out of range,
 * triangle material root, emissive material node or background index out of range).
 */
typedef struct PolarisMaterialUpdate {
	uint32_t struct_size;                       /* = sizeof(PolarisMaterialUpdate) */
	uint32_t num_material_nodes;                /* must equal the uploaded scene's */
	const PolarisMaterialNode *material_nodes;  /* [num_material_nodes]: the whole new table */
	uint32_t num_triangles;                     /* must equal the uploaded scene's when material_index is given */
	const uint32_t *material_index;             /* NULL = unchanged; else [num_triangles] root node per triangle */
	int32_t scene_diffuse_mat_index;            /* always taken: pass the uploaded value to keep it; -1 = no background */
	const uint32_t *emissive_mat_nodes;         /* NULL = unchanged; else [num_emissives]: new PolarisEmissive.mat_node_index per entry */
	uint32_t num_emissives;                     /* must equal the uploaded scene's when emissive_mat_nodes is given */
} PolarisMaterialUpdate;
int polaris_hip_update_materials(polaris_hip_tracer *h, const PolarisMaterialUpdate *u);
int polaris_hip_update_texture(polaris_hip_tracer *h, uint32_t index, const void *texels, size_t n_bytes);

/* Test tap (no reference counterpart): the device's pair records (POLARIS_REC_PAIRS: 64 bytes each, scene_layout.h PairNodeH) or
 * instance records (POLARIS_REC_INSTS: 64 bytes each, InstH) of the uploaded scene, copied back; POLARIS_REC_COUNTS: four uint64_t,
 * the number of pair records, of instance records, of device allocations the scene owns and the bytes in them (what the option
 * "instance_update" adds shows here, exactly; free device memory is everybody's); POLARIS_REC_TRIS: the triangle records (48 bytes
 * each, TriH), one per triangle slot; POLARIS_REC_SHADING: four uint32_t, tri_bits, emit_classes, the background node as bits and the
 * number of triangle slots.  n_bytes must be at least the size of what is asked for. */
#define POLARIS_REC_PAIRS 0
#define POLARIS_REC_INSTS 1
#define POLARIS_REC_COUNTS 2
#define POLARIS_REC_TRIS 3
#define POLARIS_REC_SHADING 4
int polaris_hip_read_scene_records(polaris_hip_tracer *h, int which, void *out, size_t n_bytes);

/*
 * BVH construction on the device -- an ALTERNATIVE producer of the scene's two-level BVH (the stretch; the
 * reference's own builder, asset/compiler/bvh/bvh_builder.go:100-308, scores ~1024 / (depth + 1) candidate planes per axis with
 * one goroutine each and is restated for the CPU in polaris_amd/host/scene_compiler.cpp).  Two algorithms (`algorithm`):
 *   POLARIS_BVH_SAH (0, the default)  binned surface-area heuristic, built level by level: 16 bins per axis, the cheapest of the
 *       3 x 15 planes per node (the criterion of bvh_builder.go:162-211, plane count aside), a node no plane separates is halved by
 *       position.  Frames trace within 1 % of the CPU-built tree; 1 M triangles build in ~7 ms.  Depth is bounded by
 *       the float range of the centroid extents plus log2(n) -- not by log2(n) alone: geometrically spaced outliers make a chain --
 *       and a tree deeper than the 32-entry traversal stack is refused by upload_scene, whoever built it.
 *   POLARIS_BVH_LBVH (1)  linear BVH: Morton order of the centroids (one radix sort), all inner nodes at once (Karras 2012), boxes
 *       fitted bottom-up, subtrees of up to max_leaf_tris triangles collapsed into the reference's kind of leaf.  2-6 x faster to
 *       build, deeper and looser: frames take 26-55 % longer on it, and a mesh that packs many triangles into one cell of the 30-bit
 *       grid can exceed the traversal stack (upload_scene then refuses the scene: use the SAH builder or a CPU producer).
 * One tree per mesh over its triangles, one over the instances' world boxes with one instance per leaf (compiler.go:88-103).  Output in
 * the reference's encoding (PolarisBvhNode; node 0 = the scene's root), ready for PolarisSceneView once the caller has put the
 * triangle arrays in the new order:
 *   tri_order[new position] = old triangle index (a permutation within every mesh's range; emissive tri_index values follow it);
 *   mesh_root[m] = the node a PolarisMeshInstance.bvh_root of mesh m must name.
 * nodes_capacity >= 2 * (num_instances + num_triangles).  The tree differs from the reference compiler's (another algorithm) --
 * parity is defined on the uploaded arrays, and any tree whose boxes bound their contents is traversed correctly.
 * device_ms (may be NULL) = the build on the device, vertices resident, without the read-back.  No tracer handle is involved.
 * in->struct_size must be sizeof(PolarisBvhBuildInput) (ABI 5): POLARIS_E_BAD_ARGUMENT otherwise.
 */
typedef struct PolarisBvhBuildInput {
	uint32_t struct_size;           /* = sizeof(PolarisBvhBuildInput): a caller built against another layout is refused (ABI 5) */
	const float *vertices;          /* float4 per vertex, 3 per triangle, as PolarisSceneView.vertices */
	uint32_t num_triangles;
	const uint32_t *mesh_first_tri; /* [num_meshes]: mesh m owns triangles [first, first + count); the ranges tile [0, num_triangles) in order */
	const uint32_t *mesh_num_tris;
	uint32_t num_meshes;
	const float *instance_boxes;    /* [num_instances][6]: world-space min.xyz, max.xyz of every mesh instance (the scene reader's boxes) */
	const uint32_t *instance_mesh;  /* [num_instances] */
	uint32_t num_instances;
	uint32_t max_leaf_tris;         /* 1..15 */
	uint32_t algorithm;             /* POLARIS_BVH_SAH (0, the default: binned surface-area heuristic, level by level) or POLARIS_BVH_LBVH (1: linear BVH, 2-6 x faster to build, 26-55 % slower to trace); ABI 4 */
} PolarisBvhBuildInput;
#define POLARIS_BVH_SAH 0u
#define POLARIS_BVH_LBVH 1u
int polaris_hip_build_bvh(int device, const PolarisBvhBuildInput *in, PolarisBvhNode *nodes, uint32_t nodes_capacity, uint32_t *num_nodes,
                          uint32_t *tri_order, uint32_t *mesh_root, double *device_ms);
const char *polaris_hip_build_bvh_error(void); /* text of the calling thread's last polaris_hip_build_bvh failure */

/* With option time_kernels=1: accumulated device milliseconds and launch count of the named
 * timer since the last call for that name.  Timers: "generate", "intersect_packet" (camera rays through
 * the wave-packet kernel), "intersect" (closest hit), "shade_first" / "shade_sort" /
 * "shade_plain" / "shade_wave" (one per shade kernel symbol), "scan", "occlusion", "fold" (the batch's NEE records into the
 * per-path radiance), "resolve", "aggregate", "tonemap", "gbuffer" and "denoise" (polaris_hip_set_denoise), "reproject" and "temporal"
 * (polaris_hip_set_temporal), "variance" and "denoise_variance" (polaris_hip_set_variance), "instance_extent",
 * "repad" and "refit_top" (polaris_hip_update_instances), "tri_records" and "refit_mesh" (polaris_hip_update_vertices, which runs the
 * former three as well), "retag" (polaris_hip_update_materials), "meter", "expose" and "display" (polaris_hip_set_display: with
 * it on "tonemap" does not run in a sync), "bloom" (polaris_hip_set_bloom: one bracket around all pyramid launches of a sync; the bloomed
 * display step stays under "display"). */
int polaris_hip_kernel_ms(polaris_hip_tracer *h, const char *kernel, double *ms, uint64_t *launches);

/* The kernel symbol (as rocprofv3 prints it, e.g. "pol::k_trace<false, 16, 2>") the named timer last
 * bracketed; "" if it has not run.  Measurement aid: bench.py names its roofline objects by it. */
int polaris_hip_kernel_symbol(polaris_hip_tracer *h, const char *kernel, char symbol[128]);

/* Shading events of the last Trace per bounce: counts[4 b + 0..2] = shaded hits, shaded misses, emitter
 * hits of the shade step of bounce b (their sums are PolarisTraceStats' totals), counts[4 b + 3] = which
 * shade timer that step ran under (0 shade_first, 1 shade_sort, 2 shade_plain, 3 shade_wave).
 * n_counts >= 4 * POLARIS_MAX_BOUNCES.  Measurement aid: algorithmic bytes per shade kernel symbol. */
int polaris_hip_shade_counts(polaris_hip_tracer *h, uint64_t *counts, size_t n_counts);

#ifdef __cplusplus
}
#endif
#endif /* POLARIS_HIP_H */
