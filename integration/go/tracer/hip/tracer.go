// Package hip is the MI355X (gfx950) tracer backend for polaris.  It implements
// tracer.Tracer (tracer/tracer.go:80-111) by calling the C ABI of libpolaris_hip.so
// (include/polaris_hip.h) through cgo, and replaces tracer/opencl + tracer/opencl/device.
//
// NOTE: written without a Go toolchain (the build image has none); it has not been compiled.
// Every method is a thin call into the C ABI, which is what is built and tested.
package hip

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../../polaris_amd/lib -lpolaris_hip -Wl,-rpath,${SRCDIR}/../../../../polaris_amd/lib
#include <stdlib.h>
#include "polaris_hip.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math/rand"
	"runtime"
	"sync"
	"time"
	"unsafe"

	"github.com/achilleasa/polaris/asset/scene"
	"github.com/achilleasa/polaris/tracer"
)

var (
	// Same sentinel the OpenCL backend returns (tracer/opencl/errors.go).
	ErrNoSceneData = errors.New("hip tracer: no scene data uploaded")
)

// Tracer is one MI355X behind the tracer.Tracer interface.
type Tracer struct {
	sync.Mutex
	id     string
	dev    Device
	handle *C.polaris_hip_tracer
	stats  *tracer.Stats

	// Asynchronous updates are grouped by type; the latest wins (tracer/opencl/tracer.go:150-158).
	changeBuffer map[tracer.ChangeType]interface{}
}

// NewTracer mirrors opencl.NewTracer (tracer/opencl/tracer.go:58-72).
func NewTracer(id string, dev Device) (tracer.Tracer, error) {
	return &Tracer{id: id, dev: dev, stats: &tracer.Stats{}, changeBuffer: make(map[tracer.ChangeType]interface{})}, nil
}

func (tr *Tracer) Id() string          { return tr.id }
func (tr *Tracer) Flags() tracer.Flag  { return tracer.Local }
func (tr *Tracer) Speed() uint32       { return tr.dev.Speed }
func (tr *Tracer) Stats() *tracer.Stats { return tr.stats }

func (tr *Tracer) lastError() error {
	return fmt.Errorf("hip tracer (%s): %s", tr.dev.Name, C.GoString(C.polaris_hip_last_error(tr.handle)))
}

func (tr *Tracer) check(rc C.int) error {
	switch rc {
	case C.POLARIS_OK:
		return nil
	case C.POLARIS_E_NO_SCENE_DATA:
		return ErrNoSceneData
	default:
		return tr.lastError()
	}
}

// Init creates the device-side tracer (tracer/opencl/tracer.go:95-117).
func (tr *Tracer) Init() error {
	tr.Lock()
	defer tr.Unlock()
	if rc := C.polaris_hip_create(C.int(tr.dev.Index), &tr.handle); rc != C.POLARIS_OK {
		return fmt.Errorf("hip tracer (%s): %s", tr.dev.Name, C.GoString(C.polaris_hip_last_error(nil)))
	}
	return nil
}

// Close releases every device resource (tracer/opencl/tracer.go:120-145).
func (tr *Tracer) Close() {
	tr.Lock()
	defer tr.Unlock()
	if tr.handle != nil {
		C.polaris_hip_destroy(tr.handle)
		tr.handle = nil
	}
}

// UpdateState queues a change; synchronous updates are committed at once
// (tracer/opencl/tracer.go:150-158).
func (tr *Tracer) UpdateState(mode tracer.UpdateMode, changeType tracer.ChangeType, data interface{}) (time.Duration, error) {
	tr.changeBuffer[changeType] = data
	if mode == tracer.Synchronous {
		return tr.commitChanges()
	}
	return 0, nil
}

// commitChanges mirrors tracer/opencl/tracer.go:161-192.  All scene slices are COPIED by the
// library before the call returns: no Go pointer is retained (cgo pointer rule), unlike the
// reference's CL_MEM_USE_HOST_PTR aliasing (device/buffer.go:98-104).
func (tr *Tracer) commitChanges() (time.Duration, error) {
	if len(tr.changeBuffer) == 0 {
		return 0, nil
	}
	start := time.Now()
	for changeType, data := range tr.changeBuffer {
		var err error
		switch changeType {
		case tracer.FrameDimensions:
			dims := data.([2]uint32)
			err = tr.check(C.polaris_hip_resize(tr.handle, C.uint32_t(dims[0]), C.uint32_t(dims[1])))
		case tracer.SceneData:
			err = tr.uploadScene(data.(*scene.Scene))
		case tracer.CameraData:
			cam := data.(*scene.Camera)
			eye := [3]C.float{C.float(cam.Position[0]), C.float(cam.Position[1]), C.float(cam.Position[2])}
			var fr [16]C.float
			for c := 0; c < 4; c++ { // Frustrum = TL, TR, BL, BR (asset/scene/camera.go:125-141)
				for k := 0; k < 4; k++ {
					fr[4*c+k] = C.float(cam.Frustrum[c][k])
				}
			}
			err = tr.check(C.polaris_hip_set_camera(tr.handle, &eye[0], &fr[0]))
		default:
			err = fmt.Errorf("unsupported change type %d", changeType)
		}
		if err != nil {
			return time.Since(start), err
		}
	}
	tr.changeBuffer = make(map[tracer.ChangeType]interface{})
	tr.stats.UpdateTime = time.Since(start)
	return tr.stats.UpdateTime, nil
}

// uploadScene hands the ten flat slices of scene.Scene (asset/scene/optimized_scene.go:167-190)
// to the library; the Go structs are layout-identical to include/polaris_types.h.
func (tr *Tracer) uploadScene(sc *scene.Scene) error {
	var v C.PolarisSceneView
	if n := len(sc.BvhNodeList); n > 0 {
		v.bvh_nodes, v.num_bvh_nodes = (*C.PolarisBvhNode)(unsafe.Pointer(&sc.BvhNodeList[0])), C.uint32_t(n)
	}
	if n := len(sc.MeshInstanceList); n > 0 {
		v.mesh_instances, v.num_mesh_instances = (*C.PolarisMeshInstance)(unsafe.Pointer(&sc.MeshInstanceList[0])), C.uint32_t(n)
	}
	if n := len(sc.MaterialNodeList); n > 0 {
		v.material_nodes, v.num_material_nodes = (*C.PolarisMaterialNode)(unsafe.Pointer(&sc.MaterialNodeList[0])), C.uint32_t(n)
	}
	if n := len(sc.EmissivePrimitives); n > 0 {
		v.emissives, v.num_emissives = (*C.PolarisEmissive)(unsafe.Pointer(&sc.EmissivePrimitives[0])), C.uint32_t(n)
	}
	if n := len(sc.TextureData); n > 0 {
		v.texture_data, v.texture_data_bytes = (*C.uint8_t)(unsafe.Pointer(&sc.TextureData[0])), C.uint32_t(n)
	}
	if n := len(sc.TextureMetadata); n > 0 {
		v.texture_meta, v.num_textures = (*C.PolarisTextureMetadata)(unsafe.Pointer(&sc.TextureMetadata[0])), C.uint32_t(n)
	}
	if n := len(sc.MaterialIndex); n > 0 {
		v.vertices = (*C.float)(unsafe.Pointer(&sc.VertexList[0]))
		v.normals = (*C.float)(unsafe.Pointer(&sc.NormalList[0]))
		v.uvs = (*C.float)(unsafe.Pointer(&sc.UvList[0]))
		v.material_index = (*C.uint32_t)(unsafe.Pointer(&sc.MaterialIndex[0]))
		v.num_triangles = C.uint32_t(n)
	}
	v.scene_diffuse_mat_index = C.int32_t(sc.SceneDiffuseMatIndex)
	v.scene_emissive_mat_index = C.int32_t(sc.SceneEmissiveMatIndex)
	return tr.check(C.polaris_hip_upload_scene(tr.handle, &v))
}

func toC(req *tracer.BlockRequest) C.PolarisBlockRequest {
	// tracer.BlockRequest (tracer/tracer.go:6-34) and PolarisBlockRequest have the same 12
	// fields in the same order; copied field by field to stay independent of Go's padding rules.
	return C.PolarisBlockRequest{
		frame_w: C.uint32_t(req.FrameW), frame_h: C.uint32_t(req.FrameH),
		block_x: C.uint32_t(req.BlockX), block_y: C.uint32_t(req.BlockY),
		block_w: C.uint32_t(req.BlockW), block_h: C.uint32_t(req.BlockH),
		samples_per_pixel: C.uint32_t(req.SamplesPerPixel), num_bounces: C.uint32_t(req.NumBounces),
		min_bounces_for_rr: C.uint32_t(req.MinBouncesForRR), exposure: C.float(req.Exposure),
		seed: C.uint32_t(req.Seed), accumulated_samples: C.uint32_t(req.AccumulatedSamples),
	}
}

// Trace mirrors tracer/opencl/tracer.go:194-247.  The reference draws one math/rand value per
// sample (:222) and one per bounce (pipeline.go:146), interleaved; the same draws, in the same
// order, are made here and passed down as the seed list.
func (tr *Tracer) Trace(blockReq *tracer.BlockRequest) (time.Duration, error) {
	start := time.Now()
	if _, err := tr.commitChanges(); err != nil {
		return time.Since(start), err
	}
	stride := 1 + int(blockReq.NumBounces)
	seeds := make([]C.uint32_t, int(blockReq.SamplesPerPixel)*stride)
	for s := 0; s < int(blockReq.SamplesPerPixel); s++ {
		blockReq.Seed = rand.Uint32()
		seeds[s*stride] = C.uint32_t(blockReq.Seed)
		for b := 0; b < int(blockReq.NumBounces); b++ {
			seeds[s*stride+1+b] = C.uint32_t(rand.Uint32())
		}
	}
	creq := toC(blockReq)
	var seedPtr *C.uint32_t
	if len(seeds) > 0 {
		seedPtr = &seeds[0]
	}
	if err := tr.check(C.polaris_hip_trace(tr.handle, &creq, seedPtr, C.size_t(len(seeds)), nil)); err != nil {
		return time.Since(start), err
	}
	blockReq.AccumulatedSamples += blockReq.SamplesPerPixel // tracer.go:240
	tr.stats.BlockW = blockReq.BlockW
	tr.stats.BlockH = blockReq.BlockH
	tr.stats.RenderTime = time.Since(start)
	return tr.stats.RenderTime, nil
}

// MergeOutput mirrors tracer/opencl/tracer.go:279-286.
func (tr *Tracer) MergeOutput(other tracer.Tracer, blockReq *tracer.BlockRequest) (time.Duration, error) {
	start := time.Now()
	src, ok := other.(*Tracer)
	if !ok {
		return 0, fmt.Errorf("merge failed: unsupported tracer instance")
	}
	creq := toC(blockReq)
	return time.Since(start), tr.check(C.polaris_hip_merge(tr.handle, src.handle, &creq))
}

// ResetEpoch / WaitReset order a merge from another goroutine behind this tracer's Reset stage (Trace clears the frame
// accumulator when it starts, tracer/opencl/tracer.go:208-213) without waiting for its whole Trace: read the primary's
// epoch before the frame's blocks are handed out, and WaitReset(epoch) in a secondary's worker before it merges
// (INTEGRATION.md section 3).
func (tr *Tracer) ResetEpoch() uint64 {
	var e C.uint64_t
	C.polaris_hip_reset_epoch(tr.handle, &e)
	return uint64(e)
}

// A non-nil error (POLARIS_E_TIMEOUT: the awaited Reset never came) means the block must NOT be merged: it would land on
// an accumulator that was not cleared for this frame.
func (tr *Tracer) WaitReset(epoch uint64) error {
	return tr.check(C.polaris_hip_wait_reset(tr.handle, C.uint64_t(epoch)))
}

// SyncFramebuffer mirrors tracer/opencl/tracer.go:250-276 (wait, then tone-map).
func (tr *Tracer) SyncFramebuffer(blockReq *tracer.BlockRequest) (time.Duration, error) {
	start := time.Now()
	creq := toC(blockReq)
	return time.Since(start), tr.check(C.polaris_hip_sync_framebuffer(tr.handle, &creq))
}

// DenoiseParams configures the edge-avoiding a-trous filter SyncFramebuffer runs over the running mean (PolarisDenoiseParams,
// include/polaris_hip.h; DESIGN.md section 10).  Iterations = 0 turns it off (the default); DefaultDenoise holds the settings
// chosen on the CPU restatement.
type DenoiseParams struct {
	Iterations      uint32  // K: 0 = off, 1..8
	NormalPowerLog2 uint32  // P: 0..10
	SigmaDepth      float32 // 0 = term off, else [1e-6, 1e6]
	SigmaLuminance  float32 // 0 = term off, else [1e-6, 1e6]
}

var DefaultDenoise = DenoiseParams{Iterations: 4, NormalPowerLog2: 5, SigmaDepth: 0.1, SigmaLuminance: 4.0}

// SetDenoise turns denoising of the synced frame on or off (the filter's "post-process filters" slot of
// tracer/tracer.go:108-110).  The accumulators stay the reference result; only the frame buffer shows the filtered image.
func (tr *Tracer) SetDenoise(p DenoiseParams) error {
	var c C.PolarisDenoiseParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.iterations = C.uint32_t(p.Iterations)
	c.normal_power_log2 = C.uint32_t(p.NormalPowerLog2)
	c.sigma_depth = C.float(p.SigmaDepth)
	c.sigma_luminance = C.float(p.SigmaLuminance)
	return tr.check(C.polaris_hip_set_denoise(tr.handle, &c))
}

// TemporalParams configures temporal reuse of the synced frame across camera moves (PolarisTemporalParams, include/polaris_hip.h;
// DESIGN.md section 10b).  MaxHistory = 0 turns it off (the default) and drops the history; DefaultTemporal holds the settings
// chosen on the CPU restatement.
type TemporalParams struct {
	MaxHistory      uint32  // cap on the reused sample count: 0 = off, 1..4096
	NormalThreshold float32 // a history tap needs n_i . n_j >= this, within [-1, 1]
	DepthThreshold  float32 // ... and a hit distance within this fraction, within [0, 1e6]
}

var DefaultTemporal = TemporalParams{MaxHistory: 32, NormalThreshold: 0.9, DepthThreshold: 0.1}

// SetTemporal turns temporal reuse on or off: while the camera moves (UpdateState CameraData, as the interactive renderer's
// renderer/opengl.go:294-301), SyncFramebuffer blends the running mean with the last view's, reprojected.  The accumulators stay
// the reference result; only the frame buffer shows the blend.
func (tr *Tracer) SetTemporal(p TemporalParams) error {
	var c C.PolarisTemporalParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.max_history = C.uint32_t(p.MaxHistory)
	c.normal_threshold = C.float(p.NormalThreshold)
	c.depth_threshold = C.float(p.DepthThreshold)
	return tr.check(C.polaris_hip_set_temporal(tr.handle, &c))
}

// LensParams is the thin-lens camera (PolarisLensParams, include/polaris_hip.h; DESIGN.md section 10h): a lens point is
// eye + lx U + ly V with (lx, ly) uniform in the unit disk, and every camera ray passes through its pinhole ray's point on the plane
// FocusDistance along the unit vector Axis.  U = V = 0 turns the lens off (the default).
type LensParams struct {
	FocusDistance float32    // within [1e-6, 1e30] while the lens is on
	Axis          [3]float32 // unit view axis, world space
	U, V          [3]float32 // span the aperture; |U| = |V| = the radius of a round lens
}

// SetLens sets the thin lens.  UpdateState(CameraData) does not touch it: a caller that moves the camera derives Axis, U and V from
// the new frustum (axis = normalize(TL + TR + BL + BR), u = r normalize(TR - TL), v = r normalize(TL - BL)) and calls SetLens again.
// A changed lens drops the temporal history; the caller restarts accumulation as after a camera change.
func (tr *Tracer) SetLens(p LensParams) error {
	var c C.PolarisLensParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.focus_distance = C.float(p.FocusDistance)
	for i := 0; i < 3; i++ {
		c.axis[i] = C.float(p.Axis[i])
		c.u[i] = C.float(p.U[i])
		c.v[i] = C.float(p.V[i])
	}
	return tr.check(C.polaris_hip_set_lens(tr.handle, &c))
}

// ShutterParams is the camera at shutter close (PolarisShutterParams, include/polaris_hip.h; DESIGN.md section 10j): every camera
// ray gets its own time in [0, 1) and is generated by the camera blended between the state UpdateState(CameraData) and SetLens hold
// (shutter open) and this one.  Lens is looked at only while the lens is on; its U = V = 0 closes the aperture over the interval.
type ShutterParams struct {
	Eye     [3]float32  // the eye at shutter close
	Frustum [16]float32 // the corner rays TL, TR, BL, BR at shutter close
	Lens    LensParams  // the lens at shutter close
}

// SetShutter turns the shutter on with this close state, or off with nil.  The close state belongs to the open one: UpdateState(CameraData)
// and a SetLens that changes the lens switch the shutter off, so the order of calls is camera, lens, shutter.  A changed shutter drops the
// temporal history; the caller restarts accumulation as after a camera change.
func (tr *Tracer) SetShutter(p *ShutterParams) error {
	var c C.PolarisShutterParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	if p != nil {
		c.enabled = 1
		for i := 0; i < 3; i++ {
			c.eye1[i] = C.float(p.Eye[i])
			c.axis1[i] = C.float(p.Lens.Axis[i])
			c.u1[i] = C.float(p.Lens.U[i])
			c.v1[i] = C.float(p.Lens.V[i])
		}
		for i := 0; i < 16; i++ {
			c.frustum1[i] = C.float(p.Frustum[i])
		}
		c.focus_distance1 = C.float(p.Lens.FocusDistance)
	}
	return tr.check(C.polaris_hip_set_shutter(tr.handle, &c))
}

// Projection kinds of ProjectionParams.Kind (POLARIS_PROJECTION_*).
const (
	ProjectionPerspective     = 0 // off: the frustum of UpdateState(CameraData)
	ProjectionOrthographic    = 1
	ProjectionEquirectangular = 2
)

// ProjectionParams is the camera's projection (PolarisProjectionParams, include/polaris_hip.h; DESIGN.md section 10n): an
// orthographic window through the eye, or an equirectangular (latitude-longitude) panorama around it, on an orthonormal view basis.
// Kind = ProjectionPerspective turns it off (the default); nothing else is looked at then.
type ProjectionParams struct {
	Kind                  uint32
	Axis, Right, Up       [3]float32 // world space: +Axis forward, +Right to image right, +Up to image top
	HalfWidth, HalfHeight float32    // orthographic: half extents of the window, world units
	LonRange, LatRange    float32    // equirectangular: radians spanned by the frame's width and height
}

// SetProjection sets the projection.  The eye is UpdateState(CameraData)'s, which does not touch the basis: a caller that turns the
// camera derives Axis, Right and Up from the new frustum (axis = normalize(TL + TR + BL + BR), right = normalize(TR - TL),
// up = normalize(TL - BL) made orthogonal to the axis) and calls SetProjection again.  A projection excludes the lens and the
// shutter.  A changed projection drops the G-buffer and the temporal history; the caller restarts accumulation as after a camera
// change.  (Written without a Go toolchain at hand, as the rest of this package: it has not been compiled.)
func (tr *Tracer) SetProjection(p ProjectionParams) error {
	var c C.PolarisProjectionParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.kind = C.uint32_t(p.Kind)
	for i := 0; i < 3; i++ {
		c.axis[i] = C.float(p.Axis[i])
		c.right[i] = C.float(p.Right[i])
		c.up[i] = C.float(p.Up[i])
	}
	c.half_width = C.float(p.HalfWidth)
	c.half_height = C.float(p.HalfHeight)
	c.lon_range = C.float(p.LonRange)
	c.lat_range = C.float(p.LatRange)
	return tr.check(C.polaris_hip_set_projection(tr.handle, &c))
}

// SetObjectMotion turns the option "object_motion" on or off: with it on (and temporal reuse on) the history survives an
// UpdateState(SceneData) that only moves mesh instances -- same instances, same meshes, same triangle count -- and is reprojected
// through each instance's motion (DESIGN.md section 10d).  Changing it drops the history.
func (tr *Tracer) SetObjectMotion(on bool) error {
	key := C.CString("object_motion")
	defer C.free(unsafe.Pointer(key))
	var v C.int64_t
	if on {
		v = 1
	}
	return tr.check(C.polaris_hip_set_option(tr.handle, key, v))
}

// SetInstanceUpdate turns the option "instance_update" on or off for the NEXT UpdateState(SceneData): with it on the upload keeps
// what UpdateInstances needs (DESIGN.md section 10e).
func (tr *Tracer) SetInstanceUpdate(on bool) error {
	key := C.CString("instance_update")
	defer C.free(unsafe.Pointer(key))
	var v C.int64_t
	if on {
		v = 1
	}
	return tr.check(C.polaris_hip_set_option(tr.handle, key, v))
}

// UpdateInstances moves the uploaded scene's mesh instances in place (polaris_hip_update_instances; DESIGN.md section 10e):
// invTransforms holds 16 floats per instance (column major, as scene.MeshInstance.Transform), boxes 6 floats per instance (world-space
// min.xyz, max.xyz, the scene reader's boxes), emissives the scene's emissive list with new Transform / Area values or nil to keep
// the uploaded ones.  Afterwards the tracer behaves as if the scene had been uploaded with these and its top-level BVH refit.  The
// scene must have been uploaded after SetInstanceUpdate(true); a refusal leaves the tracer as it was.  The slices are only read
// during the call (cgo rule: nothing the caller owns is retained).
func (tr *Tracer) UpdateInstances(invTransforms []float32, boxes []float32, emissives []scene.EmissivePrimitive) error {
	tr.Lock()
	defer tr.Unlock()
	if len(invTransforms)%16 != 0 || len(boxes) != len(invTransforms)/16*6 || len(invTransforms) == 0 {
		return fmt.Errorf("hip tracer (%s): UpdateInstances wants 16 matrix floats and 6 box floats per instance", tr.dev.Name)
	}
	// c is Go memory that holds Go pointers: the cgo rules allow passing &c only while what it points to is pinned
	var pin runtime.Pinner
	defer pin.Unpin()
	var c C.PolarisInstanceUpdate
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.num_mesh_instances = C.uint32_t(len(invTransforms) / 16)
	pin.Pin(&invTransforms[0])
	pin.Pin(&boxes[0])
	c.inv_transforms = (*C.float)(unsafe.Pointer(&invTransforms[0]))
	c.instance_boxes = (*C.float)(unsafe.Pointer(&boxes[0]))
	if n := len(emissives); n > 0 {
		pin.Pin(&emissives[0])
		c.emissives, c.num_emissives = (*C.PolarisEmissive)(unsafe.Pointer(&emissives[0])), C.uint32_t(n)
	}
	return tr.check(C.polaris_hip_update_instances(tr.handle, &c))
}

// SetVertexUpdate turns the option "vertex_update" on or off for the NEXT UpdateState(SceneData): with it on the upload keeps what
// UpdateVertices needs, and what UpdateInstances needs too (DESIGN.md section 10f).
func (tr *Tracer) SetVertexUpdate(on bool) error {
	key := C.CString("vertex_update")
	defer C.free(unsafe.Pointer(key))
	var v C.int64_t
	if on {
		v = 1
	}
	return tr.check(C.polaris_hip_set_option(tr.handle, key, v))
}

// UpdateVertices deforms the uploaded scene's meshes in place (polaris_hip_update_vertices; DESIGN.md section 10f): vertices holds 4
// floats per vertex, three vertices per triangle, as the scene's vertex list; boxes 6 floats per instance (world-space min.xyz,
// max.xyz of the deformed instances); normals as vertices, or nil to keep the uploaded ones; invTransforms 16 floats per instance, or
// nil to keep the current matrices; emissives the scene's emissive list with new Transform / Area values, or nil to keep the current
// ones.  Afterwards the tracer behaves as if the scene had been uploaded with these and its mesh and top-level BVHs refit.  The scene
// must have been uploaded after SetVertexUpdate(true); a refusal leaves the tracer as it was.  The slices are only read during the
// call (cgo rule: nothing the caller owns is retained).
func (tr *Tracer) UpdateVertices(vertices []float32, boxes []float32, normals []float32, invTransforms []float32, emissives []scene.EmissivePrimitive) error {
	tr.Lock()
	defer tr.Unlock()
	if len(vertices) == 0 || len(vertices)%12 != 0 || len(boxes) == 0 || len(boxes)%6 != 0 {
		return fmt.Errorf("hip tracer (%s): UpdateVertices wants 12 vertex floats per triangle and 6 box floats per instance", tr.dev.Name)
	}
	if (normals != nil && len(normals) != len(vertices)) || (invTransforms != nil && len(invTransforms) != len(boxes)/6*16) {
		return fmt.Errorf("hip tracer (%s): UpdateVertices wants as many normals as vertices and 16 matrix floats per instance", tr.dev.Name)
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	var c C.PolarisVertexUpdate
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.num_triangles = C.uint32_t(len(vertices) / 12)
	c.num_mesh_instances = C.uint32_t(len(boxes) / 6)
	pin.Pin(&vertices[0])
	pin.Pin(&boxes[0])
	c.vertices = (*C.float)(unsafe.Pointer(&vertices[0]))
	c.instance_boxes = (*C.float)(unsafe.Pointer(&boxes[0]))
	if len(normals) > 0 {
		pin.Pin(&normals[0])
		c.normals = (*C.float)(unsafe.Pointer(&normals[0]))
	}
	if len(invTransforms) > 0 {
		pin.Pin(&invTransforms[0])
		c.inv_transforms = (*C.float)(unsafe.Pointer(&invTransforms[0]))
	}
	if n := len(emissives); n > 0 {
		pin.Pin(&emissives[0])
		c.emissives, c.num_emissives = (*C.PolarisEmissive)(unsafe.Pointer(&emissives[0])), C.uint32_t(n)
	}
	return tr.check(C.polaris_hip_update_vertices(tr.handle, &c))
}

// UpdateMaterials edits the uploaded scene's materials in place (polaris_hip_update_materials; DESIGN.md section 10g): nodes is the
// whole new material node list (as many nodes as uploaded); materialIndex the root node of every triangle, or nil to keep the
// uploaded ones; sceneDiffuse the background node, always taken (-1: none); emissiveMatNodes the new MaterialNodeIndex of every
// emissive, or nil to keep the current ones.  Afterwards the tracer behaves as if the scene had been uploaded with these.  No upload
// option is needed; a refusal leaves the tracer as it was.  The slices are only read during the call.
func (tr *Tracer) UpdateMaterials(nodes []scene.MaterialNode, materialIndex []uint32, sceneDiffuse int32, emissiveMatNodes []uint32) error {
	tr.Lock()
	defer tr.Unlock()
	if len(nodes) == 0 {
		return fmt.Errorf("hip tracer (%s): UpdateMaterials wants the whole material node list", tr.dev.Name)
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	var c C.PolarisMaterialUpdate
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.num_material_nodes = C.uint32_t(len(nodes))
	pin.Pin(&nodes[0])
	c.material_nodes = (*C.PolarisMaterialNode)(unsafe.Pointer(&nodes[0]))
	if n := len(materialIndex); n > 0 {
		pin.Pin(&materialIndex[0])
		c.material_index, c.num_triangles = (*C.uint32_t)(unsafe.Pointer(&materialIndex[0])), C.uint32_t(n)
	}
	c.scene_diffuse_mat_index = C.int32_t(sceneDiffuse)
	if n := len(emissiveMatNodes); n > 0 {
		pin.Pin(&emissiveMatNodes[0])
		c.emissive_mat_nodes, c.num_emissives = (*C.uint32_t)(unsafe.Pointer(&emissiveMatNodes[0])), C.uint32_t(n)
	}
	return tr.check(C.polaris_hip_update_materials(tr.handle, &c))
}

// UpdateTexture replaces the texels of texture index in place (polaris_hip_update_texture): same format and size as uploaded.
func (tr *Tracer) UpdateTexture(index uint32, texels []byte) error {
	tr.Lock()
	defer tr.Unlock()
	if len(texels) == 0 {
		return fmt.Errorf("hip tracer (%s): UpdateTexture wants the texture's texels", tr.dev.Name)
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&texels[0])
	return tr.check(C.polaris_hip_update_texture(tr.handle, C.uint32_t(index), unsafe.Pointer(&texels[0]), C.size_t(len(texels))))
}

// VarianceParams configures variance-guided denoising (PolarisVarianceParams, include/polaris_hip.h; DESIGN.md section 10c).
// SigmaVariance = 0 turns it off (the default); DefaultVariance holds the settings chosen on the CPU restatement.
type VarianceParams struct {
	SigmaVariance float32 // sigma_v of the variance-guided luminance term: 0 = off, else within [1e-6, 1e6]
	MinSamples    uint32  // pixels with fewer effective samples take the spatial estimate, 1..64
}

var DefaultVariance = VarianceParams{SigmaVariance: 8, MinSamples: 8}

// SetVariance turns variance guidance on or off: with it on the tracer keeps the samples' squared luminance beside the
// accumulators (option "moments", set here first) and SyncFramebuffer filters by each pixel's variance estimate.  Turning it off
// leaves "moments" on.
func (tr *Tracer) SetVariance(p VarianceParams) error {
	if p.SigmaVariance != 0 {
		key := C.CString("moments")
		defer C.free(unsafe.Pointer(key))
		if err := tr.check(C.polaris_hip_set_option(tr.handle, key, 1)); err != nil {
			return err
		}
	}
	var c C.PolarisVarianceParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.sigma_variance = C.float(p.SigmaVariance)
	c.min_samples = C.uint32_t(p.MinSamples)
	return tr.check(C.polaris_hip_set_variance(tr.handle, &c))
}

// ToneOperator is the display transform's tone curve (POLARIS_TONE_*, include/polaris_hip.h).
type ToneOperator uint32

const (
	ToneReinhard ToneOperator = iota
	ToneReinhardWhite
	ToneACES
	ToneHable
)

// DisplayParams is the display transform of SyncFramebuffer (PolarisDisplayParams, include/polaris_hip.h; DESIGN.md section 10l):
// the tone operator, the transfer function and, with AutoExposure, the frame's own metered exposure.  Enabled = false is off (the
// default): the sync ends with the reference's tone-map.
type DisplayParams struct {
	Enabled        bool
	ToneOperator   ToneOperator
	SRGB           bool    // the sRGB transfer function instead of pow(1 / 2.2)
	White          float32 // the radiance ToneReinhardWhite and ToneHable map to 1
	AutoExposure   bool
	Key            float32 // the luminance the metered window's log-average is mapped to
	CompensationEV float32
	LowPermille    uint32 // the metered window: the pixels between these two quantiles of luminance
	HighPermille   uint32
	MinEV, MaxEV   float32
	Adapt          float32 // the fraction of the way to the metered exposure one sync moves, (0, 1]
}

var DefaultDisplay = DisplayParams{Enabled: true, ToneOperator: ToneReinhard, White: 4, Key: 0.18, LowPermille: 500, HighPermille: 950,
	MinEV: -16, MaxEV: 16, Adapt: 1}

// SetDisplay turns the display transform on or off.  With AutoExposure every SyncFramebuffer meters the rows it syncs and displays
// them with the metered exposure times the request's; the exposure state adapts across camera moves, scene uploads and in-place
// updates and is reset by a resize and by a SetDisplay that changes a field.  The accumulators stay the reference result.
func (tr *Tracer) SetDisplay(p DisplayParams) error {
	b := func(v bool) C.uint32_t {
		if v {
			return 1
		}
		return 0
	}
	var c C.PolarisDisplayParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.enabled = b(p.Enabled)
	c.tone_operator = C.uint32_t(p.ToneOperator)
	c.srgb = b(p.SRGB)
	c.white = C.float(p.White)
	c.auto_exposure = b(p.AutoExposure)
	c.key = C.float(p.Key)
	c.compensation_ev = C.float(p.CompensationEV)
	c.low_permille = C.uint32_t(p.LowPermille)
	c.high_permille = C.uint32_t(p.HighPermille)
	c.min_ev = C.float(p.MinEV)
	c.max_ev = C.float(p.MaxEV)
	c.adapt = C.float(p.Adapt)
	return tr.check(C.polaris_hip_set_display(tr.handle, &c))
}

// BloomParams is PolarisBloomParams: the bloom of the display transform, a bright-pass pyramid added before the tone operator.
type BloomParams struct {
	Enabled   bool
	Levels    uint32  // 1..8 pyramid levels asked for
	Threshold float32 // the displayed-linear value above which a pixel blooms
	Knee      float32 // 0..1: soft-knee fraction of Threshold
	Intensity float32 // 0..16
	Karis     bool    // weight the first downsample by 1 / (1 + luminance)
}

// DefaultBloom is polaris_amd/ctypes_api.py BLOOM_DEFAULTS.
var DefaultBloom = BloomParams{Enabled: true, Levels: 5, Threshold: 1, Knee: 0.5, Intensity: 0.25, Karis: true}

// SetBloom turns the bloom of the display transform on or off.  It is in effect only while SetDisplay has the transform on; a call
// with the transform off is stored.  A changed call touches only the bloom pyramid.  (Written without a Go toolchain at hand: not
// compiled.)
func (tr *Tracer) SetBloom(p BloomParams) error {
	b := func(v bool) C.uint32_t {
		if v {
			return 1
		}
		return 0
	}
	var c C.PolarisBloomParams
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	c.enabled = b(p.Enabled)
	c.levels = C.uint32_t(p.Levels)
	c.threshold = C.float(p.Threshold)
	c.knee = C.float(p.Knee)
	c.intensity = C.float(p.Intensity)
	c.karis = b(p.Karis)
	return tr.check(C.polaris_hip_set_bloom(tr.handle, &c))
}

// ExposureInfo is what the last SyncFramebuffer with auto-exposure on metered (PolarisExposureInfo).
type ExposureInfo struct {
	Valid    bool
	Metered  uint64  // pixels with a finite luminance of at least 2^-16
	Avg      float32 // the window's mean log2 luminance
	Log2E, E float32 // the exposure state after the sync, and the exposure it displayed with
}

// ReadExposure returns the exposure of the last metered sync and, if histogram is not nil, its 256 luminance counts.
func (tr *Tracer) ReadExposure(histogram *[256]uint32) (ExposureInfo, error) {
	var c C.PolarisExposureInfo
	c.struct_size = C.uint32_t(unsafe.Sizeof(c))
	var h *C.uint32_t
	if histogram != nil {
		h = (*C.uint32_t)(unsafe.Pointer(&histogram[0]))
	}
	if err := tr.check(C.polaris_hip_read_exposure(tr.handle, &c, h)); err != nil {
		return ExposureInfo{}, err
	}
	return ExposureInfo{Valid: c.valid != 0, Metered: uint64(c.n_metered), Avg: float32(c.avg), Log2E: float32(c.log2E), E: float32(c.E)}, nil
}

// ReadFrameBuffer is what opencl.SaveFrameBuffer reads (tracer/opencl/pipeline.go:226-232).
func (tr *Tracer) ReadFrameBuffer(pix []uint8) error {
	if len(pix) == 0 {
		return nil
	}
	return tr.check(C.polaris_hip_read_framebuffer(tr.handle, (*C.uint8_t)(unsafe.Pointer(&pix[0])), C.size_t(len(pix))))
}

// ---- one tracer per PROCESS (INTEGRATION.md section 3b): the merge as a peer read through HIP IPC --------------------------

// IpcExport turns the trace accumulator into a ring of `depth` buffers (every Trace writes the next; TraceSlot says which) and
// returns the 576-byte blob (ABI 5: it carries the exporting GPU's PCI bus id) another process opens with IpcOpen.  Plain bytes: send them over any channel.
func (tr *Tracer) IpcExport(depth uint32) ([]byte, error) {
	var x C.PolarisIpcExport
	if err := tr.check(C.polaris_hip_ipc_export(tr.handle, C.uint32_t(depth), &x)); err != nil {
		return nil, err
	}
	return C.GoBytes(unsafe.Pointer(&x), C.int(unsafe.Sizeof(x))), nil
}

// Peer is another process's trace accumulator ring, mapped on this tracer's device.
type Peer struct{ p *C.polaris_hip_peer }

func (tr *Tracer) IpcOpen(blob []byte) (*Peer, error) {
	if len(blob) != int(unsafe.Sizeof(C.PolarisIpcExport{})) {
		return nil, fmt.Errorf("hip: an IPC export is %d bytes, got %d", unsafe.Sizeof(C.PolarisIpcExport{}), len(blob))
	}
	var p *C.polaris_hip_peer
	if err := tr.check(C.polaris_hip_ipc_open(tr.handle, (*C.PolarisIpcExport)(unsafe.Pointer(&blob[0])), &p)); err != nil {
		return nil, err
	}
	return &Peer{p}, nil
}

func (tr *Tracer) IpcClose(peer *Peer) error { return tr.check(C.polaris_hip_ipc_close(tr.handle, peer.p)) }

// MergeIpc is MergeOutput from a tracer of another process: the rows of blockReq of the peer's ring slot, read where they lie.
func (tr *Tracer) MergeIpc(peer *Peer, slot uint32, blockReq *tracer.BlockRequest) (time.Duration, error) {
	start := time.Now()
	creq := toC(blockReq)
	return time.Since(start), tr.check(C.polaris_hip_merge_ipc(tr.handle, peer.p, C.uint32_t(slot), &creq))
}

// PeerInfo says what a mapped ring really is (ABI 5): the exporter's GPU by PCI bus id, whether that is this tracer's own GPU (a
// second mapping of local memory) or another one (reads cross xGMI / PCIe), and hipDeviceCanAccessPeer towards it (-1 unknown).
type PeerInfo struct {
	Pid           uint32
	PCIBusID      string
	SameDevice    int
	LocalDevice   int
	CanAccessPeer int
	HasEvents     bool
	Staged        bool // merges from this ring go through a staging strip (no peer access to its GPU): a runtime copy, then the add
}

func (p *Peer) Info() (PeerInfo, error) {
	var i C.PolarisPeerInfo
	i.struct_size = C.uint32_t(unsafe.Sizeof(i))
	if rc := C.polaris_hip_peer_info(p.p, &i); rc != C.POLARIS_OK {
		return PeerInfo{}, fmt.Errorf("hip: peer_info failed (%d)", int(rc))
	}
	return PeerInfo{Pid: uint32(i.pid), PCIBusID: C.GoString(&i.pci_bus_id[0]), SameDevice: int(i.same_device), LocalDevice: int(i.local_device),
		CanAccessPeer: int(i.can_access_peer), HasEvents: i.has_events != 0, Staged: i.staged != 0}, nil
}

// MergeBranches names the entries of MergeCounts (POLARIS_MERGE_* in polaris_hip.h).
var MergeBranches = [...]string{"local", "peer-access", "staged", "ipc-local", "ipc-peer", "ipc-unknown", "device-strip", "ipc-staged"}

// MergeCounts reports which branch the merges onto this tracer took since it was created: a staged copy where a peer read was
// expected, or a mapping of local memory where another GPU was, shows here instead of in a timing nobody can explain.
func (tr *Tracer) MergeCounts() (map[string]uint64, error) {
	var c [C.POLARIS_MERGE_BRANCHES]C.uint64_t
	if err := tr.check(C.polaris_hip_merge_counts(tr.handle, &c[0])); err != nil {
		return nil, err
	}
	out := make(map[string]uint64, len(c))
	for i, name := range MergeBranches {
		out[name] = uint64(c[i])
	}
	return out, nil
}

// TraceSlot is the ring slot the last Trace wrote (0 without a ring).
func (tr *Tracer) TraceSlot() uint32 {
	var s C.uint32_t
	C.polaris_hip_trace_slot(tr.handle, &s)
	return uint32(s)
}
