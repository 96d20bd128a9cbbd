// polaris_hip.hip -- host side of the C ABI declared in include/polaris_hip.h.
//
// Replaces the reference's Go host layer for the tracer path (tracer/opencl/tracer.go,
// pipeline.go, resources.go, buffers.go, device/*.go) with one HIP stream per tracer handle
// and NO host round trips inside a Trace: the reference ends every one of its ~21-26 launches
// per sample in clFinish and resets two ray counters from the host before every shadeHits
// (resources.go:230-238, device/kernel.go:124); here a whole batch of samples is enqueued
// back to back, live-ray counts stay on the device, and the only synchronisation is the
// one at the end of Trace (which the interface requires: Trace is synchronous).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <unistd.h>

#include "camera_state.h"
#include "device_mem.h"
#include "frame_sync.h"
#include "kernel_table.h"
#include "merge_plan.h"
#include "polaris_hip.h"
#include "reproject_io.h"
#include "trace_plan.h"

using namespace pol;

static_assert(kPlanChunk == WG && kPlanSparseGroup == kSparseGroup && kPlanTinyBlock == kTinyBlock, "trace_plan.h counts in the kernels' geometry (kernels.h)");

#ifndef POLARIS_LDS_TOP_MAX_PAIRS
#define POLARIS_LDS_TOP_MAX_PAIRS (8u * kLdsTopNodes)
#endif

namespace {

thread_local std::string g_thread_error;
std::atomic<uint64_t> g_error_seq{0};

struct KernelTimer { double ms = 0.0; uint64_t launches = 0; };

using DevPool = std::vector<DevArray<char>>; // buffers that live and die together (dev_alloc): the scene's, a pipeline's

// moving instances in place (option "instance_update", polaris_hip_update_instances).  With the option on an upload
// keeps the update plan (scene_layout.h UpdatePlan; its device copies and the kernels' scratch live in the scene's buffers and go with
// the scene) and host copies of the emissive list and the packed light geometry.  Off, it stays empty and nothing is allocated.
struct InstanceUpdateState {
	bool on = false; // the uploaded scene has a plan
	UpdatePlan plan;
	std::vector<PolarisEmissive> emissives;
	std::vector<float> light_geo;
	PairNode *pairs = nullptr; InstRec *insts = nullptr; // the scene's records, writable (these four: set by every upload)
	PolarisEmissive *d_emissives = nullptr; float *d_light_geo = nullptr;
	UpdateNode *nodes = nullptr; uint32_t *level_first = nullptr, *tri_list = nullptr; uint2 *inst_range = nullptr;
	PaddedBox *padded = nullptr; float *pads = nullptr;
	UpdateBox *scratch = nullptr; InstUpdateRec *recs = nullptr; float *partial = nullptr;
	uint32_t chunks = 1, chunk_tris = kExtentChunkTris; // k_instance_extent: chunks per instance, triangles per chunk
};

// deforming meshes in place (option "vertex_update", polaris_hip_update_vertices).  With the option on an upload keeps
// everything the instance update keeps (whose plan carries the mesh plan: scene_layout.h MeshPlan) plus the device copies below, in
// the scene's buffers like the rest, and a host copy of the current instance matrices.  Off, it stays empty.
struct VertexUpdateState {
	bool on = false; // the scene was uploaded with the option on (the mesh plan itself may still have been refused: upd.plan.mesh)
	std::vector<float> inv; // [NI][16]: the current inverse matrices (upload, update_instances and update_vertices keep it current)
	uint32_t num_triangles = 0, num_slots = 0;
	float4 *vertices = nullptr, *normals = nullptr; TriRec *tris = nullptr; // the scene's arrays, writable (set by every upload)
	uint32_t *slot_src = nullptr, *level_first = nullptr; MeshPlanNode *nodes = nullptr;
	float4 *scratch = nullptr, *mesh_box = nullptr;
};

// editing materials in place (polaris_hip_update_materials / polaris_hip_update_texture; no option): the few host-side
// numbers the calls' checks need and the scene's tables, writable.  Set by every upload; nothing is allocated for it.
struct MaterialUpdateState {
	uint32_t num_triangles = 0, num_slots = 0;
	bool meta_word = false; // the slots carry the tiny meta word (scene_layout.h: at most 2 046 slots and triangles)
	std::vector<PolarisTextureMetadata> tex_meta; // 16 B per texture
	TriRec *tris = nullptr; uint32_t *mat_index = nullptr; PolarisMaterialNode *nodes = nullptr; PolarisEmissive *emissives = nullptr; uint8_t *tex_data = nullptr;
};

// The uploaded scene (buffers.go:180-201, re-laid out by scene_layout.h): everything that lives and dies with an upload.  Every device
// pointer below points into `bufs`: assigning DeviceScene() forgets the scene, and a failed upload leaves no pointer behind.
struct DeviceScene {
	bool have_scene = false; // complete: set last by upload_scene; update_vertices and the material edits clear it while they work
	DevPool bufs;
	BvhDev bvh{};
	SceneDev scene{};
	int max_stack = 0; uint32_t num_insts = 0; // (mesh instances: the length of bvh.insts)
	int node_mode = kNodesGlobal; // where k_trace reads node records from (kernels.h NodeMode)
	bool tiny_one = false;        // tiny-scene mode: the scene is one instance whose boxes all bound their subtrees (kernels.h k_trace, ONE); option tiny_one = 0 keeps the general variant
	TraceLaunch trace[2];         // [any hit]: the scene's k_trace variant with its block size, dynamic LDS bytes and residency (select_trace)
	InstanceUpdateState upd; VertexUpdateState vup; // kept with the options "instance_update" / "vertex_update" at upload
	MaterialUpdateState mup;
};

// The display stage of polaris_hip_sync_framebuffer (polaris_hip_set_display; display.h): its params and what its kernels
// share on the device -- the histogram, the bins' values, the exposure state and the constant 1.0f -- allocated by the first displayed
// sync and freed when the stage is turned off.  reset(): the next displayed sync starts from no exposure state.  Callers hold mu.
struct DisplayStage {
	PolarisDisplayParams p{sizeof(PolarisDisplayParams), 0, 0, 0, 0.0f, 0, 0.0f, 0.0f, 0, 0, 0.0f, 0.0f, 0.0f};
	DevArray<DpDevice> dev;
	DpDevice init{};      // what a reset uploads (kept here: the copy is asynchronous)
	bool fresh = false;   // dev holds the values, the 1.0f and an exposure state no older than the last reset
	bool metered = false; // a sync with auto-exposure on ran since the last reset (polaris_hip_read_exposure)
	void reset() { fresh = metered = false; }
	DpMeter meter() const { return DpMeter{p.low_permille, p.high_permille, dp_log2_key(p.key), p.compensation_ev, p.min_ev, p.max_ev, p.adapt}; }
};
// d->init: the bins' values, the 1.0f and the exposure state a sync starts from (prev_log2E = null: none).
inline void dp_init(DpDevice &d, const float *prev_log2E) {
	d = DpDevice{};
	for (uint32_t b = 0; b < kDpBins; b++) d.value[b] = dp_bin_value(b);
	d.one = d.s.E = 1.0f;
	if (prev_log2E) { d.s.log2E = *prev_log2E; d.s.valid = 1u; }
}

// The bloom of the display stage (polaris_hip_set_bloom; bloom.h): its params and its pyramid -- every level of the
// whole frame in one allocation, made by the first bloomed sync and freed when bloom or the display goes off, by a changed set_bloom
// and by a resize.  Not a Plane: SyncState does not know it.  Callers hold mu.
struct BloomStage {
	PolarisBloomParams p{sizeof(PolarisBloomParams), 0, 0, 0.0f, 0.0f, 0.0f, 0};
	DevArray<float4> pyramid;
	int fused = 0; // the option "bloom_fused": k_bloom_tail runs the small levels in one launch (off by default: not faster at 1024 x 1024)
};

// Everything behind the features of polaris_hip_sync_framebuffer: the parameters of denoising (polaris_hip_set_denoise),
// temporal reuse across camera moves (_set_temporal) and variance guidance (_set_variance), the option "object_motion", every plane
// they use and what of the planes is valid.  frame_sync.h holds the rules: nothing is allocated while its feature is off, the history
// is the TEMPORAL plane, G-buffer, camera and (object motion) INSTANCE plane and instance table of the last temporal sync before the
// latest change, swapped in by capture().  Each member below pairs ONE transition of SyncState with the planes it frees or swaps, so
// the two cannot drift apart; nothing else assigns a validity flag.  Callers hold mu; where planes may go every stream is idle.
struct FrameSync {
	PolarisDenoiseParams dn{sizeof(PolarisDenoiseParams), 0, 0, 0.0f, 0.0f};
	PolarisTemporalParams tp{sizeof(PolarisTemporalParams), 0, 0.0f, 0.0f};
	PolarisVarianceParams va{sizeof(PolarisVarianceParams), 0.0f, 0};
	int opt_object_motion = 0;
	int opt_guide_specular = 0; // delta links the guide ray follows (0: the first hit, k_gbuffer)
	int opt_vertex_motion = 0;  // DESIGN.md 10k; it can be in effect only on a scene uploaded with "vertex_update":
	bool scene_deformable = false;
	SyncState v;
	DevArray<float4> pl[kNumPlanes4];     // the float4 planes, by Plane
	DevArray<uint32_t> gb_inst, tp_hinst; // kInst, kHInst
	DevArray<float4> mo_table;            // kMoTable
	std::vector<float> mo_table_host;
	DevArray<uint4> gb_hit;               // kHit, and what goes with it: the vertices the history was seen with ([3 NT], scene order) and the
	DevArray<float4> vert_snap, de_table; // deformation table (temporal.h tp_deform_table), both grow-only
	std::vector<float> de_table_host;
	CameraFloats tp_hcam{};               // the history's camera
	DisplayStage dp;                      // the sync's last step, with the features on or off (its state is not a plane: SyncState does not know it)
	BloomStage bl;                        // its bloom, in effect only with dp on

	SyncFeatures features() const {
		return {dn.iterations != 0, tp.max_history != 0, va.sigma_variance != 0.0f, opt_object_motion != 0, opt_vertex_motion != 0 && scene_deformable,
		        dp.p.enabled != 0, dp.p.enabled != 0 && dp.p.auto_exposure != 0, bl.p.enabled != 0};
	}
	void drop(uint32_t set) {
		for (uint32_t p = 0; p < kNumPlanes4; p++)
			if (set >> p & 1) pl[p].reset();
		if (set & kMotionPlanes) { gb_inst.reset(); tp_hinst.reset(); mo_table.reset(); } // (they go together; ensure_gbuffer recomputes the G-buffer when gb_inst is wanted and missing)
		if (set & (kMotionPlanes | kVertexMotionPlanes)) { gb_hit.reset(); vert_snap.reset(); de_table.reset(); }
	}
	void capture(uint32_t swaps, const CameraFloats &cam) { // cam: what the planes that join the history were seen under
		constexpr Plane twin[][2] = {{kTpOut, kTpHist}, {kGuide, kTpHGuide}, {kAlbedo, kTpHAlbedo}, {kVaOut, kVaHist}};
		for (auto &t : twin)
			if (swaps >> t[0] & 1) std::swap(pl[t[0]], pl[t[1]]);
		if (swaps >> kInst & 1) std::swap(gb_inst, tp_hinst);
		if (swaps) tp_hcam = cam;
	}
	void resized() { drop(v.resized()); dp.reset(); bl.pyramid.reset(); }
	void camera_moved(const CameraFloats &old) { capture(v.camera_moved(features()), old); }
	void scene_changed(const InstTable *next, const CameraFloats &cam) { capture(v.scene_changed(features(), next), cam); } // (upload_scene and the in-place updates, before they change the scene)
	void set_temporal(const PolarisTemporalParams &p) {
		if (p.max_history == 0) { if (tp.max_history) drop(v.temporal_off()); }
		else if (p.max_history != tp.max_history || pm_f2u(p.normal_threshold) != pm_f2u(tp.normal_threshold) || pm_f2u(p.depth_threshold) != pm_f2u(tp.depth_threshold))
			v.temporal_params_changed();
		tp = p;
	}
	void projection_changed() { v.guide_rule_changed(); } // the G-buffer and the history were seen through another projection (camera_state.h, kCamProjection): both go, the planes stay
	void lens_changed() { if (tp.max_history) drop(v.temporal_off()); } // the history saw another lens or shutter (camera_state.h, kCamDropHistory): it goes as with max_history = 0; the (pinhole) G-buffer stays
	void set_variance(const PolarisVarianceParams &p) {
		if ((p.sigma_variance != 0.0f) != (va.sigma_variance != 0.0f)) drop(v.variance_toggled(p.sigma_variance != 0.0f));
		va = p;
	}
	void set_object_motion(int on) { opt_object_motion = on; drop(v.motion_toggled(on != 0)); } // (on differs from the option's value)
	void set_vertex_motion(int on) { opt_vertex_motion = on; drop(v.deform_toggled(features().deform)); } // (on differs from the option's value)
	void set_scene_deformable(bool d) { // an upload, before its scene_changed: with the option on, a scene that puts it in or out of effect is a toggle
		const bool toggled = opt_vertex_motion && d != scene_deformable;
		scene_deformable = d;
		if (toggled) drop(v.deform_toggled(d));
	}
	void set_guide_specular(int links) { opt_guide_specular = links; v.guide_rule_changed(); } // (links differs from the option's value)
};

inline uint32_t grid_for(size_t n) { return (uint32_t)((n + WG - 1) / WG); }

// The two accumulators (buffers.go:127-174) with everything MergeOutput needs around them; merge_plan.h holds the rules.  The TRACE
// accumulator is a ring (polaris_hip_ipc_export): with depth > 1 every Trace writes the next slot, so a peer process may still read
// frame f's rows while frame f + 1 is traced; depth 1 is the reference's single buffer.  It belongs to the handle's mu.  Each member
// that moves the ring's index also does what the move means for the slots and their export events, so the three cannot drift apart.
// The FRAME accumulator belongs to the MERGE stream: the Reset stage, MergeOutput and merge_device run there, under `mu` below
// only -- never under the handle's mu, which a Trace holds from start to end -- so a secondary's MergeOutput onto the primary
// overlaps the primary's own Trace (Exec1DNoWait, tracer/opencl/resources.go:119; renderer/default.go:188-191 calls it from the
// secondaries' goroutines).  SyncFramebuffer makes the main stream wait for the merges queued so far.
// Lock order: the handle's mu, then mu.  W / H / frame are written under both and may be read under either.
struct FrameAccum {
	uint32_t W = 0, H = 0;
	DevArray<float4> frame;
	DevArray<float4> ring[POLARIS_IPC_MAX_DEPTH];
	RingIndex ix;
	// One inter-process event PER RING SLOT, recorded at the end of the Trace that wrote the slot (once exported).  A slot's event
	// is re-recorded only when a Trace comes round to the slot again -- which the caller's protocol forbids while a peer may still
	// read it -- so a peer's wait on slot s's event names exactly the Trace whose rows it is about to read (round 4 had ONE event
	// re-recorded by every Trace: a primary merging frame f while the peer was already in Trace f + 1 waited for whichever it got).
	DevEvent ev_done[POLARIS_IPC_MAX_DEPTH];

	DevStream q; // the merge stream
	std::mutex mu;
	DevEvent ev_merged;
	DevArray<float4> staging;                    // peer-merge staging strip (grow-only; the merge stream's: merges are serialised on it)
	uint64_t counts[POLARIS_MERGE_BRANCHES] = {}; // which branch every merge onto this tracer took (polaris_hip_merge_counts)
	std::string error;                           // last error of a merge (the handle's `error` belongs to its mu)
	uint64_t error_seq = 0;                      // (g_error_seq: which of the two is the newer one)
	int ipc_staged = 0; // option, a testing aid: peers opened from now on are merged through the staging strip (the path of a GPU without peer access)
	// Reset epoch: how many times a Trace with accumulated_samples == 0 (or reset_frame) has got as far as queueing the clear
	// of the frame accumulator -- or has failed before it could.  A host that merges from other threads waits for the
	// primary's epoch to advance before it queues this frame's merges (polaris_hip_wait_reset), instead of for the
	// primary's whole Trace.
	uint64_t reset_epoch = 0;
	std::condition_variable reset_cv;
	// Events recorded by OTHER handles' merge streams behind their reads of this handle's trace accumulator
	// (polaris_hip_merge with dst != src): this handle's next Trace waits for them before it clears the rows.
	struct Reader { DevEvent ev; int device; };
	std::mutex readers_mu;
	std::vector<Reader> readers, reader_pool;

	// ---- the ring (caller holds the handle's mu; release, resize and redepth: mu too, every stream idle)
	float4 *current() const { return ring[ix.pos]; }
	float4 *slot(int s) const { const int i = ix.slot_of(s); return i < 0 ? nullptr : ring[i].get(); } // s < 0: the current one; null: out of range (or no frame yet)
	void advance() { ix.advance(); }
	void release() { // no frame: an IPC export dies with the buffers (peers close, the tracer exports again), and its events with it
		for (auto &s : ring) s.reset();
		for (auto &e : ev_done) e.reset();
		ix.reset();
		frame.reset();
		W = H = 0;
	}
	static hipError_t alloc_cleared(DevArray<float4> &a, size_t F, hipStream_t main) {
		const hipError_t e = a.alloc(F);
		return e != hipSuccess ? e : hipMemsetAsync(a, 0, F * sizeof(float4), main);
	}
	hipError_t resize(uint32_t w, uint32_t h, hipStream_t main) { // a single cleared buffer each; the dimensions stand once all of it does
		release();
		hipError_t e = alloc_cleared(ring[0], (size_t)w * h, main);
		if (e == hipSuccess) e = alloc_cleared(frame, (size_t)w * h, main);
		if (e == hipSuccess) e = hipStreamSynchronize(main);
		if (e == hipSuccess) { W = w; H = h; }
		return e;
	}
	hipError_t redepth(uint32_t depth, hipStream_t main) { // grow or shrink the ring to `depth` slots (slot 0 always exists); new slots are cleared
		for (uint32_t i = 0; i < POLARIS_IPC_MAX_DEPTH; i++) {
			if (i >= depth) { ring[i].reset(); ev_done[i].reset(); }
			else if (!ring[i])
				if (const hipError_t e = alloc_cleared(ring[i], (size_t)W * H, main)) return e;
		}
		const hipError_t e = hipStreamSynchronize(main);
		if (e == hipSuccess) ix.redepth(depth);
		return e;
	}

	// ---- the frame accumulator and the merge stream
	// Clear the frame accumulator and announce the reset (caller holds the handle's mu, not mu).  clear = false: a Trace that failed
	// before it could queue the clear announces all the same, so that nobody waits for a reset that will not come.
	hipError_t reset_frame(bool clear = true) {
		hipError_t e = hipSuccess;
		{
			std::lock_guard<std::mutex> lk(mu);
			if (clear) e = hipMemsetAsync(frame, 0, (size_t)W * H * sizeof(float4), q);
			reset_epoch++;
		}
		reset_cv.notify_all();
		return e;
	}
	// THE launch that adds n pixels of `rows` onto the frame accumulator from pixel `off` on, counted as `branch` (caller holds mu).
	hipError_t add_rows(const float4 *rows, size_t off, size_t n, bool moments, int branch) {
		kAggregate[moments].enqueue(grid_for(n), WG, 0, q, rows, frame + off, (uint32_t)n);
		const hipError_t e = hipGetLastError();
		if (e == hipSuccess) counts[branch]++;
		return e;
	}
	bool need_staging(size_t n) { // the staging strip, big enough for n pixels (caller holds mu)
		if (staging.capacity() >= n) return true;
		(void)hipStreamSynchronize(q); // (an earlier merge may still read the strip that goes)
		return staging.alloc(n) == hipSuccess;
	}
	int fail(int code, const char *msg) { // a merge's error (caller holds mu; the handle's `error` belongs to its mu, which a running Trace holds)
		error = msg;
		error_seq = ++g_error_seq;
		g_thread_error = msg;
		return code;
	}
	// Everything queued on the merge stream so far happens before whatever is queued on `main` next (caller holds the handle's mu).
	hipError_t join_merges(hipStream_t main) {
		std::lock_guard<std::mutex> lk(mu);
		hipError_t e = hipEventRecord(ev_merged, q);
		if (e == hipSuccess) e = hipStreamWaitEvent(main, ev_merged, 0);
		return e;
	}

	// ---- other handles' reads of the trace accumulator
	// Whatever other handles' merge streams still read of the trace accumulator happens before what is queued on `main` next (caller
	// holds the handle's mu).  The events go back to the pool: a later record simply re-arms them.
	hipError_t wait_readers(hipStream_t main) {
		std::lock_guard<std::mutex> lk(readers_mu);
		hipError_t first = hipSuccess;
		for (auto &r : readers) {
			const hipError_t e = hipStreamWaitEvent(main, r.ev, 0);
			if (first == hipSuccess) first = e;
			reader_pool.push_back(std::move(r));
		}
		readers.clear();
		return first;
	}
	// An event on `device` (the current device) for a read of the trace accumulator; recorded by the reader, then handed back (add_reader).
	DevEvent reader_event(int device) {
		std::lock_guard<std::mutex> lk(readers_mu);
		for (size_t i = 0; i < reader_pool.size(); i++)
			if (reader_pool[i].device == device) {
				DevEvent e = std::move(reader_pool[i].ev);
				reader_pool.erase(reader_pool.begin() + (long)i);
				return e;
			}
		DevEvent e;
		if (e.create(hipEventCreateWithFlags, hipEventDisableTiming) != hipSuccess) (void)hipGetLastError();
		return e;
	}
	void add_reader(DevEvent e, int device) {
		std::lock_guard<std::mutex> lk(readers_mu);
		readers.push_back({std::move(e), device});
	}
};

} // namespace

// Every stream, event and device allocation of the handle is a member that owns it (device_mem.h), so `delete h` releases
// them all and a new one needs no line in polaris_hip_destroy, which only makes every stream idle first.  The members'
// destruction order (the reverse of their declaration) means nothing: with every stream idle no handle depends on another.
struct polaris_hip_tracer {
	int device = 0;
	char pci_bus_id[32] = {}; // which GPU `device` is (device indices are per process); "" if the runtime does not say
	hipStream_t stream = nullptr; // the main stream: an alias of pipe[0].q, which owns it
	std::mutex mu;
	std::string error;
	uint64_t error_seq = 0; // (g_error_seq: whether `error` or fa.error is the newer one)

	FrameAccum fa; // the trace accumulator's ring, the frame accumulator and the merge stream (whose lock fa.mu is taken after mu)
	DevArray<uchar4> framebuffer;

	// the uploaded scene, and the options the next upload resolves into it
	DeviceScene ds;
	int opt_node_mode = -1;       // -1 = by scene size
	int opt_tiny_one = 1;
	int opt_lds_tris = -1;        // tiny-scene mode: triangle records kept in LDS; -1 = as many as fit, 0 = none (A/B aid)

	CameraState camera; // camera, lens and shutter as the caller sent them (tracer.go:175-179; camera_state.h holds the setters' rules)

	FrameSync fs; // the synced frame's features, planes and history
	int opt_instance_update = 0, opt_vertex_update = 0; // the in-place updates: the next upload keeps what they need in ds.upd / ds.vup
	std::atomic<bool> opt_moments{false}; // option "moments" (the accumulators' .w keeps the sum of L^2; variance guidance needs it): merges read it under fa.mu, hence atomic

	// wavefront batch state: up to kMaxPipes pipelines (option "overlap", default 4; a Trace uses min(overlap, #batches) of
	// them) so that consecutive batches overlap: the sparse late-bounce launches of batch i run beside the dense early
	// bounces of batch i+1 on another stream
	struct Pipe {
		DevStream q; // (pipe[0].q is the main stream)
		size_t slots = 0; // capacity in slots
		Streams st{};
		// batched mode: one NEE record array (occ_e) and one shadow-ray count array (cnt_occ) PER BOUNCE, kept until k_fold_nee has
		// added the batch's unoccluded records to the per-path radiance (kernels.h, nee_unoccluded); [0] are st.occ_e / st.cnt_occ
		float4 *nee[POLARIS_MAX_BOUNCES] = {};
		uint8_t *vis[POLARIS_MAX_BOUNCES] = {};
		uint32_t *cnt_occ_b[POLARIS_MAX_BOUNCES] = {};
		uint32_t nee_bounces = 0; // how many of them are allocated
		DevPool bufs;
		DevEvent done; // recorded after the pipe's last resolve
		void release() { // forget everything the pipe owned (its stream must be idle)
			bufs.clear();
			st = Streams{};
			slots = 0;
			nee_bounces = 0;
			for (auto &x : nee) x = nullptr;
			for (auto &x : vis) x = nullptr;
			for (auto &x : cnt_occ_b) x = nullptr;
		}
	};
	static constexpr int kMaxPipes = pol::kMaxPipes;
	Pipe pipe[kMaxPipes];
	DevArray<uint32_t> d_seeds; // grow-only
	DevArray<unsigned long long> d_stats;
	DevArray<float4> d_cam_o; // eye | FLT_MAX: the one origin record of every camera ray (launch_trace, camera)
	int num_cus = 256;
	int shade_wave_resident[2] = {5, 5}; // [LDS tables]: workgroups of k_shade_wave a CU holds at once (occupancy API, at creation)
	DevArray<uint32_t> d_retag; // polaris_hip_update_materials: the class of every material node (a byte each), then the emissives' new nodes (grow-only)

	// options: what a Trace plans from (trace_plan.h), and the rest
	TraceOptions opt;
	bool packet_primary = true;  // opt.packet_primary, resolved at upload where it is -1
	int opt_time_kernels = 0;
	int opt_max_leaf_tris = -1;   // subdivide bigger triangle leaves at upload (0 = keep the caller's leaves, -1 = by scene size)

	// per-kernel timing (option time_kernels)
	struct Pending { const char *name; DevEvent a, b; };
	std::vector<Pending> pending;
	std::vector<Pending> merge_pending; // launches on the merge stream (under fa.mu)
	std::vector<DevEvent> event_pool;
	std::map<std::string, KernelTimer> timers;
	std::map<std::string, const char *> timer_symbol; // timer name -> the kernel symbol it last bracketed (polaris_hip_kernel_symbol)
	int last_shade_timer[POLARIS_MAX_BOUNCES] = {};            // per bounce of the last Trace: 0 shade_first, 1 shade_sort, 2 shade_plain, 3 shade_wave
	uint64_t last_shade_counts[3 * POLARIS_MAX_BOUNCES] = {}; // per bounce of the last Trace: shaded hits, shaded misses, emitter hits
	DevEvent ev_start, ev_stop, ev_fork;
};

// Another process's trace accumulator ring, opened through HIP IPC on `owner`'s device.
struct polaris_hip_peer {
	polaris_hip_tracer *owner = nullptr;
	uint32_t depth = 0, W = 0, H = 0;
	IpcMapping mem[POLARIS_IPC_MAX_DEPTH];
	DevEvent ev[POLARIS_IPC_MAX_DEPTH];        // per slot: the peer's "the Trace that wrote this slot is done" event (null: the exporter had none)
	PolarisPeerInfo info{};                    // what the mapping is (polaris_hip_peer_info); info.same_device picks the merge branch counted
	void drop_events() { for (auto &e : ev) e.reset(); } // under owner->fa.mu once the peer is published
};


namespace {

int fail(polaris_hip_tracer *h, int code, const char *fmt, ...) {
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	if (h) { h->error = buf; h->error_seq = ++g_error_seq; }
	g_thread_error = buf;
	return code;
}

#define HIP_TRY(h, expr)                                                                              \
	do {                                                                                              \
		hipError_t e_ = (expr);                                                                       \
		if (e_ != hipSuccess) return fail(h, POLARIS_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
	} while (0)

template <typename T>
int dev_alloc(polaris_hip_tracer *h, DevPool &pool, T **out, size_t count) {
	DevArray<char> a;
	HIP_TRY(h, a.alloc(std::max<size_t>(count * sizeof(T), 16)));
	*out = (T *)a.get();
	pool.push_back(std::move(a));
	return POLARIS_OK;
}

template <typename T>
int dev_upload(polaris_hip_tracer *h, DevPool &pool, T **out, const void *src, size_t count) {
	int rc = dev_alloc(h, pool, out, count);
	if (rc) return rc;
	if (count) HIP_TRY(h, hipMemcpyAsync(*out, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
	return POLARIS_OK;
}

// Bracket a launch with events when time_kernels is on (name = null: never), and note the symbol the timer brackets.
struct Timed {
	polaris_hip_tracer *h;
	const char *name;
	hipStream_t q;
	bool on_merge; // a launch on the merge stream: the caller holds fa.mu (not mu), so the event pool is not touched
	DevEvent a, b;
	Timed(polaris_hip_tracer *h_, const char *n, const char *symbol, hipStream_t q_, bool merge = false) : h(h_), name(n), q(q_), on_merge(merge) {
		if (!h->opt_time_kernels || !name) return;
		if (symbol) h->timer_symbol[name] = symbol; // (null: a bracket around no kernel, or one on the merge stream -- the map belongs to mu)
		auto get = [&]() {
			DevEvent e;
			if (!on_merge && !h->event_pool.empty()) { e = std::move(h->event_pool.back()); h->event_pool.pop_back(); }
			else (void)e.create(hipEventCreate);
			return e;
		};
		a = get(); b = get();
		if (a) (void)hipEventRecord(a, q);
	}
	~Timed() {
		if (!a || !b) return;
		(void)hipEventRecord(b, q);
		(on_merge ? h->merge_pending : h->pending).push_back({name, std::move(a), std::move(b)});
	}
};

// THE launch of a kernel on stream q, bracketed by the named timer, which remembers the variant's symbol; returns the launch's error (also left for hipGetLastError).
template <class... P, class... A>
hipError_t launch(polaris_hip_tracer *h, const char *timer, hipStream_t q, const Variant<P...> &v, dim3 grid, uint32_t block, uint32_t lds_bytes, A &&...a) {
	Timed t(h, timer, v.symbol, q);
	v.enqueue(grid, block, lds_bytes, q, std::forward<A>(a)...);
	return hipPeekAtLastError();
}

void collect_timers(polaris_hip_tracer *h) { // caller holds mu; the main stream must be idle
	auto take = [&](std::vector<polaris_hip_tracer::Pending> &list, bool may_be_running) {
		std::vector<polaris_hip_tracer::Pending> keep;
		for (auto &p : list) {
			float ms = 0.0f;
			const hipError_t e = hipEventElapsedTime(&ms, p.a, p.b);
			if (e == hipErrorNotReady && may_be_running) { (void)hipGetLastError(); keep.push_back(std::move(p)); continue; }
			if (e == hipSuccess) {
				auto &t = h->timers[p.name];
				t.ms += ms;
				t.launches++;
			}
			h->event_pool.push_back(std::move(p.a));
			h->event_pool.push_back(std::move(p.b));
		}
		list.swap(keep);
	};
	take(h->pending, false);
	std::lock_guard<std::mutex> lk(h->fa.mu); // (another thread may be queueing a merge right now: its events stay pending)
	take(h->merge_pending, true);
}

hipError_t sync_all(polaris_hip_tracer *h) { // every pipeline of the handle idle (before anything the kernels use is freed)
	hipError_t first = h->fa.q ? hipStreamSynchronize(h->fa.q) : hipSuccess;
	for (int p = 0; p < polaris_hip_tracer::kMaxPipes; p++)
		if (h->pipe[p].q) {
			const hipError_t e = hipStreamSynchronize(h->pipe[p].q);
			if (first == hipSuccess) first = e;
		}
	return first;
}

int ensure_streams(polaris_hip_tracer *h, int p, size_t slots, bool want_inst, uint32_t nee_bounces = 1) {
	polaris_hip_tracer::Pipe &P = h->pipe[p];
	nee_bounces = std::max(1u, std::min<uint32_t>(nee_bounces, POLARIS_MAX_BOUNCES));
	if (slots <= P.slots && (!want_inst || P.st.hit_inst) && nee_bounces <= P.nee_bounces) return POLARIS_OK;
	slots = std::max(slots, P.slots);
	nee_bounces = std::max(nee_bounces, P.nee_bounces);
	HIP_TRY(h, hipStreamSynchronize(P.q));
	P.release();
	const size_t wgs = slots / WG;
	int rc = 0;
	rc |= dev_alloc(h, P.bufs, &P.st.ray_o, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.ray_d, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.thr, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.hit, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.occ_o, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.occ_d, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.occ_e, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.lsum, slots);
	rc |= dev_alloc(h, P.bufs, &P.st.cnt_ray, wgs);
	rc |= dev_alloc(h, P.bufs, &P.st.cnt_occ, wgs);
	rc |= dev_alloc(h, P.bufs, &P.st.pfx, wgs);
	rc |= dev_alloc(h, P.bufs, &P.st.wg_stat, wgs);
	rc |= dev_alloc(h, P.bufs, &P.st.emask[0], wgs * 8);
	rc |= dev_alloc(h, P.bufs, &P.st.emask[1], wgs * 8);
	if (want_inst) rc |= dev_alloc(h, P.bufs, &P.st.hit_inst, slots);
	P.nee[0] = P.st.occ_e;
	P.cnt_occ_b[0] = P.st.cnt_occ;
	rc |= dev_alloc(h, P.bufs, &P.vis[0], slots);
	P.st.vis = P.vis[0];
	for (uint32_t b = 1; b < nee_bounces; b++) {
		rc |= dev_alloc(h, P.bufs, &P.nee[b], slots);
		rc |= dev_alloc(h, P.bufs, &P.vis[b], slots);
		rc |= dev_alloc(h, P.bufs, &P.cnt_occ_b[b], wgs);
	}
	if (rc) { P.release(); return rc; } // (nothing was queued on the stream since it was synchronised above)
	P.slots = slots;
	P.nee_bounces = nee_bounces;
	return POLARIS_OK;
}

// A block refusal (merge_plan.h refuse_block) in words, by BlockRefusal; null: the caller's own (a call under mu names the numbers, a merge does not).
const char *const kBlockRefusal[] = {nullptr, "block request is null", "frame dimensions not set (UpdateState FrameDimensions)", nullptr, nullptr,
                                     "only full-width row blocks are supported (BlockW = FrameW, renderer/default.go:110)"};

int check_request(polaris_hip_tracer *h, const PolarisBlockRequest *r) {
	switch (const BlockRefusal why = refuse_block(h->fa.W, h->fa.H, r)) {
	case BlockRefusal::None: return POLARIS_OK;
	case BlockRefusal::FrameMismatch: return fail(h, POLARIS_E_BAD_ARGUMENT, "request frame %ux%u does not match the tracer's %ux%u", r->frame_w, r->frame_h, h->fa.W, h->fa.H);
	case BlockRefusal::RowsOutside: return fail(h, POLARIS_E_BAD_ARGUMENT, "block rows [%u,%u) outside the frame", r->block_y, r->block_y + r->block_h);
	default: return fail(h, POLARIS_E_BAD_ARGUMENT, "%s", kBlockRefusal[(int)why]);
	}
}

// The kernels' arguments of the handle's camera for its W x H frame: the open camera and lens, and the shutter's close ones (what a
// generator does not read is not looked at).  The only place the texel is computed (resources.go:130-133); the close camera
// carries the open one's, which is all k_generate_shutter reads.
struct CameraDev { CameraArgs cam, cam1; LensArgs lens, lens1; };
CameraDev camera_args(const polaris_hip_tracer *h) {
	const CameraState &c = h->camera;
	const float2 texel = make_float2(1.0f / (float)h->fa.W, 1.0f / (float)h->fa.H);
	auto cam = [&](const float *eye, const float *f) {
		return CameraArgs{make_float4(f[0], f[1], f[2], f[3]), make_float4(f[4], f[5], f[6], f[7]), make_float4(f[8], f[9], f[10], f[11]),
		                  make_float4(f[12], f[13], f[14], f[15]), make_float3(eye[0], eye[1], eye[2]), texel};
	};
	auto lens = [](const float *f) { // the ten floats: focus distance, axis, u, v
		return LensArgs{f[0], make_float3(f[1], f[2], f[3]), make_float3(f[4], f[5], f[6]), make_float3(f[7], f[8], f[9])};
	};
	return {cam(c.open.eye, c.open.frustum), cam(c.shutter.eye1, c.shutter.frustum1), lens(&c.lens.focus_distance), lens(&c.shutter.focus_distance1)};
}
// The projection of the handle's camera as the kernels and temporal.h take it (polaris_hip_set_projection is on): the basis and the two
// extents of the kind in force.
TpProjection projection_args(const CameraState &c) {
	const PolarisProjectionParams &p = c.projection;
	const bool ortho = p.kind == POLARIS_PROJECTION_ORTHOGRAPHIC;
	return TpProjection{p.kind, {p.axis[0], p.axis[1], p.axis[2]}, {p.right[0], p.right[1], p.right[2]}, {p.up[0], p.up[1], p.up[2]},
	                    ortho ? p.half_width : p.lon_range, ortho ? p.half_height : p.lat_range};
}

// The planes of the set `need` exist from their first use on, each of the frame's size; those of `clear` are cleared on the main stream,
// those of `clear_new` if they are allocated here (caller holds mu).
int ensure_planes(polaris_hip_tracer *h, uint32_t need, uint32_t clear = 0, uint32_t clear_new = 0) {
	FrameSync &S = h->fs;
	const size_t F = (size_t)h->fa.W * h->fa.H;
	for (uint32_t p = 0; p < kNumPlanes4; p++) {
		if (!(need >> p & 1)) continue;
		if (!S.pl[p]) { HIP_TRY(h, S.pl[p].alloc(F)); clear |= clear_new & 1u << p; }
		if (clear >> p & 1) HIP_TRY(h, hipMemsetAsync(S.pl[p], 0, F * sizeof(float4), h->stream));
	}
	if ((need >> kInst & 1) && !S.gb_inst) HIP_TRY(h, S.gb_inst.alloc(F));
	if ((need >> kHit & 1) && !S.gb_hit) HIP_TRY(h, S.gb_hit.alloc(F));
	return POLARIS_OK;
}

// The GUIDE / ALBEDO planes of the current scene, camera and frame size (with object motion in effect the INSTANCE plane too, with vertex
// motion in effect the HIT plane), computed
// if they are not (caller holds mu; checks done).
int ensure_gbuffer(polaris_hip_tracer *h) {
	FrameSync &S = h->fs;
	const bool want_inst = S.features().motion_on(), want_hit = S.features().deform_on();
	if (S.v.gbuffer() && (!want_inst || S.gb_inst) && (!want_hit || S.gb_hit)) return POLARIS_OK;
	const size_t F = (size_t)h->fa.W * h->fa.H;
	if (int rc = ensure_planes(h, planes(kGuide, kAlbedo) | (want_inst ? planes(kInst) : 0) | (want_hit ? planes(kHit) : 0))) return rc;
	const CameraArgs cam = camera_args(h).cam;
	uint32_t *const inst = want_inst ? S.gb_inst.get() : nullptr;
	uint4 *const hit = want_hit ? S.gb_hit.get() : nullptr;
	if (h->camera.projection_on()) { //  the same planes from the projected camera's guide rays
		const GbufferProjCamera pc{TpProjCamera{projection_args(h->camera), {cam.eye.x, cam.eye.y, cam.eye.z}}, cam.texel};
		if (S.opt_guide_specular == 0)
			(void)launch(h, "gbuffer", h->stream, kGbufferProj, grid_for(F), WG, 0, h->ds.bvh, h->ds.scene, pc, h->fa.W, (uint32_t)F, S.pl[kGuide], S.pl[kAlbedo], inst, hit);
		else
			(void)launch(h, "gbuffer", h->stream, kGbufferChainProj, grid_for(F), WG, 0, h->ds.bvh, h->ds.scene, pc, h->fa.W, (uint32_t)F, S.pl[kGuide], S.pl[kAlbedo],
			             inst, hit, S.opt_guide_specular);
	} else if (S.opt_guide_specular == 0)
		(void)launch(h, "gbuffer", h->stream, kGbuffer, grid_for(F), WG, 0, h->ds.bvh, h->ds.scene, cam, h->fa.W, (uint32_t)F, S.pl[kGuide], S.pl[kAlbedo],
		             want_inst ? S.gb_inst.get() : nullptr, want_hit ? S.gb_hit.get() : nullptr);
	else
		(void)launch(h, "gbuffer", h->stream, kGbufferChain, grid_for(F), WG, 0, h->ds.bvh, h->ds.scene, cam, h->fa.W, (uint32_t)F, S.pl[kGuide],
		             S.pl[kAlbedo], want_inst ? S.gb_inst.get() : nullptr, want_hit ? S.gb_hit.get() : nullptr, S.opt_guide_specular);
	HIP_TRY(h, hipGetLastError());
	S.v.gbuffer_computed();
	return POLARIS_OK;
}

// The option "object_motion" was turned on after the upload: the scene's matrices come back from the device's instance records (rows 0-2
// of inv_transform, all the traversal and the motion table use); the mesh indices do not (InstTable::topology_known).  Main stream idle.
int read_back_instances(polaris_hip_tracer *h) {
	std::vector<InstH> recs(h->ds.num_insts);
	HIP_TRY(h, hipMemcpy(recs.data(), h->ds.bvh.insts, recs.size() * sizeof(InstH), hipMemcpyDeviceToHost));
	InstTable &cur = h->fs.v.cur;
	cur.mesh_index.assign(h->ds.num_insts, 0u);
	cur.inv.assign((size_t)h->ds.num_insts * 16, 0.0f);
	for (uint32_t i = 0; i < h->ds.num_insts; i++) {
		float *m = cur.inv.data() + 16 * (size_t)i; // column major: m[4 * c + r]
		for (int c = 0; c < 4; c++) { m[4 * c + 0] = recs[i].r0[c]; m[4 * c + 1] = recs[i].r1[c]; m[4 * c + 2] = recs[i].r2[c]; }
		m[15] = 1.0f;
	}
	return POLARIS_OK;
}

// The record of the scene's one top-level instance travels in the kernel arguments: its matrix rows from the layout's or an update's record.
template <class Rec>
void set_root_inst(BvhDev &bvh, const Rec &I) {
	bvh.root_inst.r0 = make_float4(I.r0[0], I.r0[1], I.r0[2], I.r0[3]);
	bvh.root_inst.r1 = make_float4(I.r1[0], I.r1[1], I.r1[2], I.r1[3]);
	bvh.root_inst.r2 = make_float4(I.r2[0], I.r2[1], I.r2[2], I.r2[3]);
}

// The scene's k_trace variants (closest hit, any hit) into the handle: STACK from the exact depth the scene needs, NODES from its
// size (kernels.h, NodeMode), ONE in the tiny-scene mode; with the workgroup size.  plan_tiny_lds and trace_occupancy fill in the rest.
void select_trace(polaris_hip_tracer *h) {
	const bool tiny = h->ds.node_mode == kNodesLdsAll;
	for (int any = 0; any < 2; any++)
		h->ds.trace[any] = TraceLaunch{tiny ? &kTraceTiny[any][h->ds.tiny_one] : &kTrace[any][h->ds.max_stack <= 16 ? 0 : (h->ds.max_stack <= 24 ? 1 : 2)][h->ds.node_mode == kNodesLdsTop],
		                            tiny ? kTinyBlock : WG, 0, 6};
}

// The scene's k_trace variant over `chunks` chunks of st on stream q, under `timer` (null: a probe's launch, untimed).  camera: the closest-hit launch of a batch's
// camera rays -- their common origin comes from the handle's one-record buffer (kernels.h k_trace, o_mask), the origin stream is neither written nor read for them.
hipError_t launch_trace(polaris_hip_tracer *h, const char *timer, bool any_hit, hipStream_t q, Streams st, uint32_t grid, uint32_t chunks, float4 *acc, bool camera = false) {
	const TraceLaunch &T = h->ds.trace[any_hit];
	uint32_t o_mask = ~0u;
	if (camera && !any_hit) { st.ray_o = h->d_cam_o; o_mask = 0u; }
	return launch(h, timer, q, *T.v, grid, (uint32_t)T.block, T.lds_bytes, st, h->ds.bvh, chunks, acc, h->d_stats, o_mask);
}

// Tiny-scene mode: lay out the dynamic LDS block of a k_trace workgroup for the uploaded scene (kernels.h, k_trace) -- the stack
// rows its tree needs, its pair records, and as many triangle records (slots in descending order of how often their leaf is
// reached, scene_layout.h) as still fit while TWO workgroups share a CU's LDS, which the occupancy query confirms.
int plan_tiny_lds(polaris_hip_tracer *h, size_t n_slots) {
	// (no dummy row: the bytes in front of the stack serve; a scene that IS one instance is entered at ray set-up without an exit
	// marker, which the layout's stack need counts)
	const uint32_t rows = (uint32_t)std::max(1, h->ds.max_stack - (h->ds.bvh.root_is_instance ? 1 : 0));
	constexpr uint32_t kRowBytes = kTinyBlock * (uint32_t)sizeof(int16_t), kTriBytes = 9 * sizeof(float) + sizeof(uint32_t);
	const uint32_t nodes = h->ds.bvh.num_pairs * (uint32_t)sizeof(PairNode);
	hipDeviceProp_t prop;
	size_t lds_per_cu = 160 * 1024;
	if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.maxSharedMemoryPerMultiProcessor > 0) lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
	const size_t half = lds_per_cu / 2;
	const size_t slack = 256; // the kernel's static LDS (work cursor, dummy arrays)
	auto stack_off = [&](uint32_t tris) { return std::max<uint32_t>(kRowBytes, (nodes + tris * kTriBytes + 15u) & ~15u); };
	if (stack_off(0) + rows * kRowBytes + slack > half) return fail(h, POLARIS_E_DEVICE, "tiny-scene mode: stack and tree do not fit half a CU's LDS (%zu bytes)", half);
	uint32_t tris = (uint32_t)std::min<size_t>(n_slots, (half - slack - rows * kRowBytes - nodes - 16) / kTriBytes);
	// a wave with lanes on both fetch paths pays for both: below half of the slots the LDS copy costs more than it saves (measured:
	// 150 of the Cornell box's 808 slots +2 % frame time, 300 -1.5 %, 532 -3.5 %)
	if (tris < n_slots / 2) tris = 0;
	if (h->opt_lds_tris >= 0) tris = std::min<uint32_t>(tris, (uint32_t)h->opt_lds_tris);
	for (;;) {
		h->ds.bvh.tiny_stack_off = stack_off(tris);
		h->ds.bvh.lds_tris = tris;
		h->ds.trace[0].lds_bytes = h->ds.trace[1].lds_bytes = h->ds.bvh.tiny_stack_off + rows * kRowBytes;
		int worst = 8;
		for (const TraceLaunch &T : h->ds.trace) {
			// (the attribute belongs to the kernel, not to this handle: always the most any scene may ask for, so that handles
			// with different scenes in one process do not lower it under each other)
			HIP_TRY(h, hipFuncSetAttribute(T.v->address(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(half - slack)));
			int n = 0;
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, T.v->address(), T.block, T.lds_bytes) != hipSuccess) { (void)hipGetLastError(); n = 2; } // (no answer: trust the arithmetic)
			worst = std::min(worst, n);
		}
		if (worst >= 2 || tris == 0) break;
		tris = tris > 32 ? tris - 32 : 0; // the allocation granularity was coarser than assumed: give some back
	}
	if (getenv("POLARIS_DEBUG")) fprintf(stderr, "[polaris] tiny mode: %u stack rows at %u, %u pair records, %u of %zu triangle records in LDS (%u bytes per workgroup)\n", rows, h->ds.bvh.tiny_stack_off, h->ds.bvh.num_pairs, h->ds.bvh.lds_tris, n_slots, h->ds.trace[0].lds_bytes);
	return POLARIS_OK;
}

// Resident workgroups per CU of the scene's k_trace variant.
int trace_occupancy(polaris_hip_tracer *h, bool any_hit) {
	const TraceLaunch &T = h->ds.trace[any_hit];
	int n = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, T.v->address(), T.block, T.lds_bytes) != hipSuccess || n < 1) n = h->ds.node_mode == kNodesLdsAll ? 1 : (h->ds.max_stack <= 24 ? 6 : 5);
	if (getenv("POLARIS_DEBUG")) fprintf(stderr, "[polaris] k_trace<%d> node mode %d: %d resident workgroups of %d threads per CU\n", (int)any_hit, h->ds.node_mode, n, T.block);
	return std::min(n, 8);
}

// Resident workgroups per CU of k_shade_wave<lds>: its persistent grid is exactly what the GPU holds at once (trace_plan.h, shade_wave_grid).
int shade_wave_occupancy(bool lds) {
	int n = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kShadeWave[lds].address(), WG, 0) != hipSuccess || n < 1) { (void)hipGetLastError(); n = POLARIS_SHADE_WAVE_WAVES; } // (no answer: the kernel's waves per SIMD = its four-wave workgroups per CU)
	if (getenv("POLARIS_DEBUG")) fprintf(stderr, "[polaris] k_shade_wave<%d>: %d resident workgroups of %d threads per CU\n", (int)lds, n, (int)WG);
	return std::min(n, 8);
}

// What a Trace's plan needs to know of the uploaded scene and of the device (trace_plan.h, which holds every rule): filled here only.
TraceScene plan_scene(const polaris_hip_tracer *h) {
	TraceScene s;
	s.tiny = h->ds.node_mode == kNodesLdsAll;
	for (int any = 0; any < 2; any++) s.resident_per_cu[any] = h->ds.trace[any].resident_per_cu;
	s.tables_fit_lds = h->ds.scene.num_nodes <= kLdsMatNodes && h->ds.scene.num_emissives <= kLdsLights && h->ds.scene.num_textures <= kLdsTextures;
	s.emit_classes = h->ds.scene.emit_classes;
	s.tri_bits = h->ds.scene.tri_bits;
	s.packet_primary = h->packet_primary;
	s.num_cus = h->num_cus;
	for (int lds = 0; lds < 2; lds++) s.shade_wave_resident[lds] = h->shade_wave_resident[lds];
	s.lens = h->camera.lens_on();
	s.shutter = h->camera.shutter_on();
	s.projection = h->camera.projection_on();
	return s;
}

// THE launch of a traversal over `chunks` chunks of st, by the kernel the plan chose for the ray set (trace_plan.h: batch_traversal,
// probe_traversal, tap_traversal), under `timer` (null: a probe's or the tap's launch, untimed).  persistent_grid: k_trace's grid.
hipError_t launch_traversal(polaris_hip_tracer *h, const char *timer, Traversal how, RayKind kind, hipStream_t q, const Streams &st, uint32_t persistent_grid, uint32_t chunks, float4 *acc) {
	const bool any_hit = kind == RayKind::AnyHit;
	if (how == Traversal::Packet)
		return launch(h, timer, q, kPacket[any_hit ? kPacketAnyHit : (kind == RayKind::Camera ? kPacketCamera : kPacketClosest)], chunks, WG, 0, st, h->ds.bvh, acc, h->d_stats, make_float3(h->camera.open.eye[0], h->camera.open.eye[1], h->camera.open.eye[2]));
	if (how == Traversal::Persistent) return launch_trace(h, timer, any_hit, q, st, persistent_grid, chunks, acc, kind == RayKind::Camera);
	if (any_hit) return launch(h, timer, q, kOcclusion, chunks, WG, 0, st, h->ds.bvh, acc, h->d_stats);
	return launch(h, timer, q, kIntersect, chunks, WG, 0, st, h->ds.bvh);
}

// THE launch of the camera's generator (camera_state.h Generator) over `wgs` workgroups of st: the rays of samples first_sample.. of the
// seed list with `stride` seeds per sample, rows from block_y, under `timer` (null: the tap's launch, untimed).  write_origin: the pinhole's alone.
hipError_t launch_generate(polaris_hip_tracer *h, const char *timer, hipStream_t q, const Streams &st, uint32_t stride, uint32_t first_sample, uint32_t wgs, uint32_t N,
                           uint32_t Npad, uint32_t block_y, int zero_lsum, int write_origin) {
	const CameraDev c = camera_args(h);
	const uint32_t *seeds = h->d_seeds;
	switch (const Generator g = h->camera.generator()) {
	case Generator::Pinhole: return launch(h, timer, q, kGenerate, wgs, WG, 0, st, c.cam, seeds, stride, first_sample, N, Npad, h->fa.W, block_y, zero_lsum, write_origin);
	case Generator::Ortho: case Generator::Equirect:
		return launch(h, timer, q, kGenerateProj[g == Generator::Equirect], wgs, WG, 0, st, projection_args(h->camera), c.cam.eye, c.cam.texel, seeds, stride, first_sample, N,
		              Npad, h->fa.W, block_y, zero_lsum);
	case Generator::Lens: return launch(h, timer, q, kGenerateLens, wgs, WG, 0, st, c.cam, c.lens, seeds, stride, first_sample, N, Npad, h->fa.W, block_y, zero_lsum);
	default: return launch(h, timer, q, kGenerateShutter[g == Generator::ShutterLens], wgs, WG, 0, st, c.cam, c.cam1, c.lens, c.lens1, seeds, stride, first_sample, N, Npad, h->fa.W, block_y, zero_lsum);
	}
}

const char *const kShadeTimer[4] ={"shade_first", "shade_sort", "shade_plain", "shade_wave"}; // by ShadeKernel (trace_plan.h): one timer per kernel symbol

// One wavefront batch: K samples starting at sample s0, on pipeline p, by the Trace's plan.
// Returns the first launch error of the batch (checked after every batch by the caller: a failed launch in batch 1 is reported
// before batch 2 is queued behind it).
hipError_t launch_batch(polaris_hip_tracer *h, int p, const PolarisBlockRequest *r, const TracePlan &plan, uint32_t s0, uint32_t K, uint32_t N, hipEvent_t resolve_after) {
	hipError_t first_err = hipSuccess;
	auto note = [&](hipError_t e) { if (first_err == hipSuccess && e != hipSuccess) first_err = e; };
	polaris_hip_tracer::Pipe &P = h->pipe[p];
	const bool exact = plan.exact;
	const uint32_t B = plan.bounces, stride = 1 + B, Npad = plan.Npad;
	const uint32_t wgs_per_sample = Npad / WG, wgs = K * wgs_per_sample;
	hipStream_t q = P.q;
	P.st.hit12 = plan.hit12 ? 1u : 0u; // (a Trace never reads a hit's distance: kernels.h Streams::hit12)
	P.st.o12 = plan.o12 ? 1u : 0u;     // (... and its closest-hit rays all have the max distance FLT_MAX: Streams::o12)
	note(launch_generate(h, "generate", q, P.st, stride, s0, wgs, N, Npad, r->block_y, exact ? 0 : 1, plan.generate_writes_origins ? 1 : 0));
	ShadeArgs A{};
	A.seeds = h->d_seeds; A.seed_stride = stride; A.first_sample = s0;
	A.N = N; A.Npad = Npad; A.W = h->fa.W; A.blockY = r->block_y;
	A.min_rr = r->min_bounces_for_rr;
	A.exact = exact ? 1 : 0;
	A.prefilter = plan.prefilter ? 1 : 0;
	A.acc = exact ? h->fa.current() : P.st.lsum;
	const uint32_t persistent = plan.trace_grid(false, wgs), persistent_occl = plan.trace_grid(true, wgs);
	for (uint32_t b = 0; b < B; b++) {
		const BouncePlan &pl = plan.bounce[b];
		Streams S = P.st; // (in place: k_shade / k_shade_wave read a chunk's rays before they write into it)
		if (!exact) { S.occ_e = P.nee[b]; S.vis = P.vis[b]; S.cnt_occ = P.cnt_occ_b[b]; } // this bounce's NEE records, visibility bytes and shadow-ray counts stay until k_fold_nee
		float4 *const occl_acc = exact ? A.acc : nullptr;                // batched: unoccluded rays only mark their record (deferred)
		const RayKind closest = b == 0 ? plan.primary : RayKind::Closest;
		note(launch_traversal(h, traversal_timer(pl.isect, closest), pl.isect, closest, q, S, persistent, wgs, nullptr));
		A.bounce = b;
		A.last_bounce = (b + 1 == B) ? 1 : 0;
		A.emask_in = b == 0 ? nullptr : P.st.emask[(b + 1) & 1]; // the masks the previous step wrote
		A.emask_out = P.st.emask[b & 1];
		if (pl.shade == kShadeByWave) note(launch(h, kShadeTimer[pl.shade], q, kShadeWave[plan.staged], plan.shade_wave_grid(wgs), WG, 0, S, h->ds.scene, A, wgs));
		else note(launch(h, kShadeTimer[pl.shade], q, kShade[plan.staged][pl.shade], wgs, WG, 0, S, h->ds.scene, A));
		note(launch(h, "scan", q, kScan, K, 1024, 0, S, wgs_per_sample, b, A.last_bounce ? 0 : 1, h->d_stats));
		note(launch_traversal(h, traversal_timer(pl.occl, RayKind::AnyHit), pl.occl, RayKind::AnyHit, q, S, persistent_occl, wgs, occl_acc));
	}
	if (!exact && B > 0) { // accumulateEmissiveSamples of the whole batch: the marked NEE records of every bounce into the per-path radiance
		FoldArgs F{};
		for (uint32_t b = 0; b < B; b++) { F.nee[b] = P.nee[b]; F.vis[b] = P.vis[b]; F.cnt[b] = P.cnt_occ_b[b]; }
		F.bounces = B;
		note(launch(h, "fold", q, kFoldNee, wgs, WG, 0, F, P.st.lsum));
	}
	if (!exact) {
		// batches resolve into the trace accumulator in sample order: wait for the previous batch's resolve
		if (resolve_after) note(hipStreamWaitEvent(q, resolve_after, 0));
		note(launch(h, "resolve", q, kResolve[plan.moments], grid_for(N), WG, 0, P.st.lsum, h->fa.current(), K, N, Npad, r->block_y * h->fa.W));
	}
	note(hipEventRecord(P.done, q));
	note(hipGetLastError()); // (whatever a launch left)
	return first_err;
}

// ---- the scene: upload_scene's steps and what the in-place updates share (caller holds mu).  First: nothing of the handle may still run
int make_idle(polaris_hip_tracer *h) {
	HIP_TRY(h, hipSetDevice(h->device));
	HIP_TRY(h, sync_all(h));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return POLARIS_OK;
}

// Upload, step 1: the scene re-laid out for the kernels, with the plans the update options ask for.
int layout_scene(polaris_hip_tracer *h, const PolarisSceneView &sc, SceneLayout &L) {
	// Defaults by scene size (measured): small scenes live in L2/LDS and are bound by
	// instruction issue -> small leaves and packet traversal of camera rays pay; scenes far larger than
	// the caches are bound by node fetches -> fewer, fuller leaves and one ray per lane.
	const int max_leaf = h->opt_max_leaf_tris >= 0 ? h->opt_max_leaf_tris : (sc.num_triangles <= 32768u ? 2 : 4);
	std::string err;
	for (int leaf_tris : {max_leaf, 0}) { // (0: without subdivision, where the deeper tree would not fit the traversal stack)
		L = SceneLayout();
		L.want_update_plan = h->opt_instance_update != 0;
		L.want_mesh_plan = h->opt_vertex_update != 0;
		err = build_layout(sc, L, leaf_tris);
		if (err != "@retry-without-subdivision") break;
	}
	return err.empty() ? POLARIS_OK : fail(h, POLARIS_E_BAD_SCENE, "%s", err.c_str());
}

// Upload, step 3: the layout's records and the scene's arrays into h->ds.  geo: the packed light records.  The copies are only queued.
int upload_arrays(polaris_hip_tracer *h, const PolarisSceneView &sc, const SceneLayout &L, const std::vector<float> &geo) {
	DeviceScene &S = h->ds;
	int rc = 0;
	PairNode *pairs; int2 *leaves; TriRec *tris; InstRec *insts;
	rc |= dev_upload(h, S.bufs, &pairs, L.pairs.data(), L.pairs.size());
	rc |= dev_upload(h, S.bufs, &leaves, L.leaves.data(), L.leaves.size());
	rc |= dev_upload(h, S.bufs, &tris, L.tris.data(), L.tris.size());
	rc |= dev_upload(h, S.bufs, &insts, L.insts.data(), L.insts.size());
	float4 *vertices, *normals; float2 *uvs; uint32_t *mat_index;
	PolarisMaterialNode *nodes; PolarisEmissive *emissives; PolarisTextureMetadata *tex_meta; uint8_t *tex_data; float *light_geo;
	const size_t nv = (size_t)sc.num_triangles * 3;
	rc |= dev_upload(h, S.bufs, &vertices, sc.vertices, nv);
	rc |= dev_upload(h, S.bufs, &normals, sc.normals, nv);
	rc |= dev_upload(h, S.bufs, &uvs, sc.uvs, nv);
	rc |= dev_upload(h, S.bufs, &mat_index, sc.material_index, sc.num_triangles);
	rc |= dev_upload(h, S.bufs, &nodes, sc.material_nodes, sc.num_material_nodes);
	rc |= dev_upload(h, S.bufs, &emissives, sc.emissives, sc.num_emissives);
	rc |= dev_upload(h, S.bufs, &tex_meta, sc.texture_meta, sc.num_textures);
	rc |= dev_upload(h, S.bufs, &light_geo, geo.data(), geo.size());
	// the texture blob, padded: texels are fetched as the three dwords at their address whatever the format (shading.h, tex_fetch)
	rc |= dev_alloc(h, S.bufs, &tex_data, (size_t)sc.texture_data_bytes + 16);
	if (rc) return rc;
	if (sc.texture_data_bytes) HIP_TRY(h, hipMemcpyAsync(tex_data, sc.texture_data, sc.texture_data_bytes, hipMemcpyHostToDevice, h->stream));
	S.bvh = BvhDev{pairs, (uint32_t)L.pairs.size(), leaves, tris, insts, L.root_ref, 0, InstRec{}, 0, 0};
	if (L.root_ref < 0 && (((uint32_t)~L.root_ref) & 15u) == 0u && !(((uint32_t)~L.root_ref) & kBigLeafFlag)) { // the top-level tree is a single leaf ...
		const size_t root_inst = ((uint32_t)~L.root_ref) >> 4; // (... which, in the top-level tree, is an instance: its id is in the reference)
		if (root_inst < L.insts.size()) { // its record goes with the kernel arguments
			const InstH &I = L.insts[root_inst];
			S.bvh.root_is_instance = 1;
			set_root_inst(S.bvh, I);
			S.bvh.root_inst.meta = make_int4(I.root_ref, (int)I.rank, (int)I.pad[0], 0);
		}
	}
	S.scene = SceneDev{vertices, normals, uvs, mat_index, nodes, emissives, tex_meta, tex_data, sc.num_emissives,
	                   sc.scene_diffuse_mat_index, sc.num_material_nodes, sc.num_textures, light_geo, sc.num_emissives ? pm_rcp((float)(int)sc.num_emissives) : 0.0f, L.tri_bits, L.emit_classes};
	S.max_stack = L.max_stack; S.num_insts = (uint32_t)L.insts.size();
	S.upd.pairs = pairs; S.upd.insts = insts; S.upd.d_emissives = emissives; S.upd.d_light_geo = light_geo; // what the in-place updates write
	S.vup.vertices = vertices; S.vup.normals = normals; S.vup.tris = tris;
	S.mup.num_triangles = sc.num_triangles; S.mup.num_slots = (uint32_t)L.tris.size();
	S.mup.meta_word = L.tris.size() <= 2046u && sc.num_triangles <= 2046u; // (build_layout's condition for TriH::pad2)
	S.mup.tex_meta.assign(sc.texture_meta, sc.texture_meta + sc.num_textures);
	S.mup.tris = tris; S.mup.mat_index = mat_index; S.mup.nodes = nodes; S.mup.emissives = emissives; S.mup.tex_data = tex_data;
	return POLARIS_OK;
}

// Upload, step 4: what the in-place updates keep (options instance_update / vertex_update, else nothing) -- the plans' device copies and
// their kernels' scratch in the scene's buffers, the host copies (out of L and geo) in h->ds.upd / vup.  Waits for every copy of the upload.
int keep_update_plans(polaris_hip_tracer *h, const PolarisSceneView &sc, SceneLayout &L, std::vector<float> &geo) {
	DeviceScene &S = h->ds;
	InstanceUpdateState &U = S.upd; VertexUpdateState &V = S.vup;
	const uint32_t NI = sc.num_mesh_instances;
	int rc = 0;
	std::vector<uint2> inst_range;
	if (L.want_update_plan) {
		const UpdatePlan &P = L.plan;
		uint32_t longest = 1;
		inst_range.resize(NI);
		for (uint32_t i = 0; i < NI; i++) {
			const uint32_t m = P.mesh_of_inst[i];
			inst_range[i] = make_uint2(P.tri_first[m], P.tri_first[m + 1] - P.tri_first[m]);
			longest = std::max(longest, inst_range[i].y);
		}
		U.chunks = std::max(1u, std::min(std::min((longest + kExtentChunkTris - 1) / kExtentChunkTris, kExtentMaxChunks), (1u << 22) / NI));
		U.chunk_tris = (longest + U.chunks - 1) / U.chunks;
		rc |= dev_upload(h, S.bufs, &U.nodes, P.nodes.data(), P.nodes.size());
		rc |= dev_upload(h, S.bufs, &U.level_first, P.level_first.data(), P.level_first.size());
		rc |= dev_upload(h, S.bufs, &U.tri_list, P.tri_list.data(), P.tri_list.size());
		rc |= dev_upload(h, S.bufs, &U.inst_range, inst_range.data(), inst_range.size());
		rc |= dev_upload(h, S.bufs, &U.padded, P.padded.data(), P.padded.size());
		rc |= dev_alloc(h, S.bufs, &U.pads, P.mesh_box.size());
		rc |= dev_alloc(h, S.bufs, &U.scratch, P.nodes.size());
		rc |= dev_alloc(h, S.bufs, &U.recs, (size_t)NI);
		rc |= dev_alloc(h, S.bufs, &U.partial, (size_t)NI * U.chunks * 6);
	}
	if (L.want_mesh_plan && L.plan.mesh.on) {
		const MeshPlan &M = L.plan.mesh;
		rc |= dev_upload(h, S.bufs, &V.slot_src, M.slot_src.data(), M.slot_src.size());
		rc |= dev_upload(h, S.bufs, &V.nodes, M.nodes.data(), M.nodes.size());
		rc |= dev_upload(h, S.bufs, &V.level_first, M.level_first.data(), M.level_first.size());
		rc |= dev_alloc(h, S.bufs, &V.scratch, 2 * M.nodes.size());
		rc |= dev_alloc(h, S.bufs, &V.mesh_box, 2 * M.root.size());
	}
	if (rc) return rc;
	HIP_TRY(h, hipStreamSynchronize(h->stream)); // (inst_range dies at return, the plan's vectors move, L and geo go with the caller)
	if (L.want_mesh_plan) {
		V.on = true;
		V.num_triangles = sc.num_triangles;
		V.num_slots = (uint32_t)L.tris.size();
		V.inv.resize((size_t)NI * 16);
		for (uint32_t i = 0; i < NI; i++) memcpy(V.inv.data() + 16 * (size_t)i, sc.mesh_instances[i].inv_transform, 16 * sizeof(float));
	}
	if (L.want_update_plan) {
		U.on = true;
		U.plan = std::move(L.plan);
		U.emissives.assign(sc.emissives, sc.emissives + sc.num_emissives);
		U.light_geo = std::move(geo);
	}
	return POLARIS_OK;
}

// Upload, step 5: how this scene is traversed -- node mode, tiny-scene mode, the k_trace variants with LDS block and residency, packet use.
int choose_traversal(polaris_hip_tracer *h, const PolarisSceneView &sc, const SceneLayout &L) {
	DeviceScene &S = h->ds;
	// camera rays: the wave-packet kernel where a packet stays together AND the tree is small -- one instance, up to 32 K
	// triangles.  Since the per-ray kernel's instruction diet the two are level on the tiny scenes (headline 11.37 /
	// 11.31 / 11.39 ms with packets against 11.42 / 11.32 / 11.38 without, round 4: the packet kernel stays there, it keeps the
	// origin stream unwritten); on the 58 K-triangle ball the packet's dependent scalar node fetches cost more than the per-ray
	// kernel's gathers (camera rays 5.5 vs 4.1 ms per 32 spp, frame -1.8 %); in a scene of many instances the packet's lanes part
	// ways inside the instances (-5 % frame time per-ray on the 1 024-instance scene, -26 % on the 1 M-triangle terrain)
	// (round 4, later: with the triangle records in LDS the per-ray kernel of the tiny-scene mode is ahead -- camera rays 0.93 vs
	// 1.20 ms isolated, frame 10.96 vs 11.03 ms, three alternating runs: see below, after the node mode is known)
	if (h->opt.packet_primary < 0) h->packet_primary = sc.num_triangles <= 32768u && sc.num_mesh_instances == 1;
	// node records: whole tree in LDS for tiny scenes, its top for small ones, global memory otherwise (kernels.h NodeMode)
	// (16-bit stack entries: triangle slots and instance ids must fit 11 bits, and no leaf reference may carry kBigLeafFlag)
	// (... and the packed word of a slot holds the scene triangle in 11 bits too: scene_layout.h tiny_meta_word)
	const bool tiny_ok = L.pairs.size() <= (size_t)kTinyPairs && L.tris.size() <= kTinyMaxIndex && sc.num_triangles <= kTinyMaxIndex && L.insts.size() <= kTinyMaxIndex &&
	                     L.big_leaves == 0 && L.max_stack <= 16;
	S.node_mode = tiny_ok ? kNodesLdsAll : (L.pairs.size() <= (size_t)(POLARIS_LDS_TOP_MAX_PAIRS) ? kNodesLdsTop : kNodesGlobal);
	if (h->opt_node_mode >= 0 && (h->opt_node_mode != kNodesLdsAll || tiny_ok)) S.node_mode = h->opt_node_mode;
	S.tiny_one = S.node_mode == kNodesLdsAll && h->opt_tiny_one && S.bvh.root_is_instance && L.unbounded_boxes == 0;
	select_trace(h);
	if (S.node_mode == kNodesLdsAll) {
		if (int rc = plan_tiny_lds(h, L.tris.size())) return rc;
		if (h->opt.packet_primary < 0 && S.bvh.lds_tris > 0) h->packet_primary = false;
	}
	for (int any = 0; any < 2; any++) S.trace[any].resident_per_cu = trace_occupancy(h, any != 0);
	return POLARIS_OK;
}

// A refit kernel over the levels of its plan (level_first: the host copy): ONE workgroup looping over them, or a launch per level.
template <class Kernel, class Args>
void launch_levels(polaris_hip_tracer *h, const char *timer, hipStream_t q, const Kernel &kernel, const Args &A, const std::vector<uint32_t> &level_first, bool one_group) {
	const uint32_t levels = (uint32_t)level_first.size() - 1;
	if (one_group) (void)launch(h, timer, q, kernel, 1, kRefitBlock, 0, A, 0u, levels);
	else
		for (uint32_t l = 0; l < levels; l++) // (at most kTraversalStack + 1 levels: build_layout refuses a deeper tree)
			(void)launch(h, timer, q, kernel, (level_first[l + 1] - level_first[l] + kRefitBlock - 1) / kRefitBlock, kRefitBlock, 0, A, l, 1u);
}

// The device part of a vertex update on the main stream: the new arrays, the triangle records and the mesh trees' boxes from them, and
// the deformed meshes' root boxes back into the plan -- a term of the padding of the boxes leaf subdivision added (subdivision_pad).
int refit_meshes(polaris_hip_tracer *h, const PolarisVertexUpdate *u) {
	InstanceUpdateState &U = h->ds.upd; VertexUpdateState &V = h->ds.vup;
	const MeshPlan &M = U.plan.mesh;
	hipStream_t q = h->stream;
	const size_t nv = (size_t)V.num_triangles * 3;
	HIP_TRY(h, hipMemcpyAsync(V.vertices, u->vertices, nv * sizeof(float4), hipMemcpyHostToDevice, q));
	if (u->normals) HIP_TRY(h, hipMemcpyAsync(V.normals, u->normals, nv * sizeof(float4), hipMemcpyHostToDevice, q));
	(void)launch(h, "tri_records", q, kTriRecords, (V.num_slots + kTriRecordBlock - 1) / kTriRecordBlock, kTriRecordBlock, 0, V.vertices, V.slot_src, V.num_slots, V.tris);
	const MeshRefitArgs A{V.nodes, V.level_first, V.slot_src, V.vertices, V.scratch, U.pairs, U.padded, V.mesh_box};
	launch_levels(h, "refit_mesh", q, kRefitMesh, A, M.level_first, M.nodes.size() <= kMeshRefitOneGroupNodes);
	HIP_TRY(h, hipGetLastError());
	std::vector<float> boxes(8 * M.root.size());
	HIP_TRY(h, hipMemcpyAsync(boxes.data(), V.mesh_box, boxes.size() * sizeof(float), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipStreamSynchronize(q));
	for (size_t m = 0; m < M.root.size(); m++) {
		memcpy(U.plan.mesh_box[m].min, boxes.data() + 8 * m, 12);
		memcpy(U.plan.mesh_box[m].max, boxes.data() + 8 * m + 4, 12);
	}
	return POLARIS_OK;
}

// The end the two in-place updates share, on the main stream: the per-instance records, the paddings and -- geo not empty -- the
// emissives (ems; null: the kept ones) with their packed light records go to the device; then the instance refit; when it is done,
// the one-instance scene's record in the kernel arguments and the host copies of emissives and light records follow.
int finish_update(polaris_hip_tracer *h, const std::vector<InstUpdateRec> &recs, const std::vector<float> &pads, const PolarisEmissive *ems, std::vector<float> &geo) {
	InstanceUpdateState &U = h->ds.upd;
	hipStream_t q = h->stream;
	HIP_TRY(h, hipMemcpyAsync(U.recs, recs.data(), recs.size() * sizeof(InstUpdateRec), hipMemcpyHostToDevice, q));
	if (!pads.empty()) HIP_TRY(h, hipMemcpyAsync(U.pads, pads.data(), pads.size() * sizeof(float), hipMemcpyHostToDevice, q));
	if (!geo.empty()) {
		HIP_TRY(h, hipMemcpyAsync(U.d_emissives, ems ? ems : U.emissives.data(), U.emissives.size() * sizeof(PolarisEmissive), hipMemcpyHostToDevice, q));
		HIP_TRY(h, hipMemcpyAsync(U.d_light_geo, geo.data(), geo.size() * sizeof(float), hipMemcpyHostToDevice, q));
	}
	// the world extent of every instance's mesh, the padding of the boxes leaf subdivision added, the top-level refit
	const UpdatePlan &P = U.plan;
	const uint32_t NI = h->ds.num_insts;
	(void)launch(h, "instance_extent", q, kInstanceExtent, dim3(U.chunks, std::min(NI, 65535u)), kExtentBlock, 0, h->ds.scene.vertices, U.tri_list, U.inst_range, U.recs, NI, U.chunk_tris, U.partial);
	if (!P.padded.empty())
		(void)launch(h, "repad", q, kRepad, ((uint32_t)P.padded.size() + kRefitBlock - 1) / kRefitBlock, kRefitBlock, 0, U.padded, (uint32_t)P.padded.size(), U.pads, U.pairs);
	const RefitArgs A{U.nodes, U.level_first, U.scratch, U.pairs, U.insts, U.recs, U.partial, U.chunks};
	launch_levels(h, "refit_top", q, kRefitTop, A, P.level_first, P.nodes.size() <= kRefitOneGroupNodes);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipStreamSynchronize(q)); // (the arguments may go at return)
	collect_timers(h);
	if (h->ds.bvh.root_is_instance) set_root_inst(h->ds.bvh, recs[((uint32_t)~h->ds.bvh.root_ref) >> 4]);
	if (ems) U.emissives.assign(ems, ems + U.emissives.size());
	if (!geo.empty()) U.light_geo = std::move(geo);
	return POLARIS_OK;
}

} // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int polaris_hip_abi_version(void) { return POLARIS_HIP_ABI_VERSION; }

int polaris_hip_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int polaris_hip_device_info(int index, char name[256], uint32_t *compute_units, uint32_t *clock_mhz, uint64_t *global_mem_bytes) {
	int n = polaris_hip_device_count();
	if (index < 0 || index >= n) return fail(nullptr, POLARIS_E_NO_DEVICE, "device %d out of range (%d devices)", index, n);
	hipDeviceProp_t p;
	HIP_TRY(nullptr, hipGetDeviceProperties(&p, index));
	if (name) { strncpy(name, p.name, 255); name[255] = 0; }
	if (compute_units) *compute_units = (uint32_t)p.multiProcessorCount;
	if (clock_mhz) *clock_mhz = (uint32_t)(p.clockRate / 1000);
	if (global_mem_bytes) *global_mem_bytes = (uint64_t)p.totalGlobalMem;
	return POLARIS_OK;
}

int polaris_hip_device_identity(int index, PolarisDeviceIdentity *out) {
	if (!out) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "device_identity: out is null");
	if (out->struct_size != sizeof(PolarisDeviceIdentity))
		return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "device_identity: struct_size %u, this library's PolarisDeviceIdentity has %zu bytes", out->struct_size, sizeof(PolarisDeviceIdentity));
	const int n = polaris_hip_device_count();
	if (index < 0 || index >= n) return fail(nullptr, POLARIS_E_NO_DEVICE, "device %d out of range (%d devices)", index, n);
	hipDeviceProp_t p;
	HIP_TRY(nullptr, hipGetDeviceProperties(&p, index));
	memset(out, 0, sizeof *out);
	out->struct_size = sizeof *out;
	out->hip_index = index;
	if (hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof out->pci_bus_id, index) != hipSuccess) { (void)hipGetLastError(); out->pci_bus_id[0] = 0; }
	hipUUID u;
	if (hipDeviceGetUuid(&u, index) == hipSuccess) memcpy(out->uuid, u.bytes, 16);
	else (void)hipGetLastError();
	out->compute_units = (uint32_t)p.multiProcessorCount;
	out->clock_mhz = (uint32_t)(p.clockRate / 1000);
	out->global_mem_bytes = (uint64_t)p.totalGlobalMem;
	snprintf(out->name, sizeof out->name, "%s", p.name);
	snprintf(out->gcn_arch, sizeof out->gcn_arch, "%s", p.gcnArchName);
	return POLARIS_OK;
}

int polaris_hip_can_access_peer(int device, int peer_device, int *can) {
	if (!can) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "can_access_peer: out is null");
	*can = 0;
	const int n = polaris_hip_device_count();
	if (device < 0 || device >= n || peer_device < 0 || peer_device >= n) return fail(nullptr, POLARIS_E_NO_DEVICE, "can_access_peer: device %d / %d out of range (%d devices)", device, peer_device, n);
	if (device == peer_device) return POLARIS_OK;
	HIP_TRY(nullptr, hipDeviceCanAccessPeer(can, device, peer_device));
	return POLARIS_OK;
}

int polaris_hip_create(int device_index, polaris_hip_tracer **out) {
	if (!out) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "out handle pointer is null");
	*out = nullptr;
	int n = polaris_hip_device_count();
	if (device_index < 0 || device_index >= n)
		return fail(nullptr, POLARIS_E_NO_DEVICE, "device %d out of range (%d HIP devices visible)", device_index, n);
	polaris_hip_tracer *h = new polaris_hip_tracer();
	h->device = device_index;
	if (hipDeviceGetPCIBusId(h->pci_bus_id, (int)sizeof h->pci_bus_id, device_index) != hipSuccess) { (void)hipGetLastError(); h->pci_bus_id[0] = 0; }
	hipError_t e = hipSetDevice(device_index);
	for (int p = 0; p < polaris_hip_tracer::kMaxPipes && e == hipSuccess; p++) e = h->pipe[p].q.create(hipStreamCreateWithFlags, hipStreamNonBlocking);
	h->stream = h->pipe[0].q;
	for (int p = 0; p < polaris_hip_tracer::kMaxPipes && e == hipSuccess; p++) e = h->pipe[p].done.create(hipEventCreateWithFlags, hipEventDisableTiming);
	if (e == hipSuccess) e = h->ev_fork.create(hipEventCreateWithFlags, hipEventDisableTiming);
	if (e == hipSuccess) e = h->fa.q.create(hipStreamCreateWithFlags, hipStreamNonBlocking);
	if (e == hipSuccess) e = h->fa.ev_merged.create(hipEventCreateWithFlags, hipEventDisableTiming);
	if (e == hipSuccess) e = h->d_stats.alloc(ST_COUNT);
	if (e == hipSuccess) e = h->d_cam_o.alloc(1);
	if (e == hipSuccess) {
		hipDeviceProp_t p;
		if (hipGetDeviceProperties(&p, device_index) == hipSuccess && p.multiProcessorCount > 0) h->num_cus = p.multiProcessorCount;
		for (int lds = 0; lds < 2; lds++) h->shade_wave_resident[lds] = shade_wave_occupancy(lds != 0);
	}
	if (e == hipSuccess) e = h->ev_start.create(hipEventCreate);
	if (e == hipSuccess) e = h->ev_stop.create(hipEventCreate);
	if (e != hipSuccess) {
		fail(nullptr, POLARIS_E_DEVICE, "creating tracer on device %d: %s", device_index, hipGetErrorString(e));
		delete h; // (releases whatever was created before the failure)
		return POLARIS_E_DEVICE;
	}
	*out = h;
	return POLARIS_OK;
}

void polaris_hip_destroy(polaris_hip_tracer *h) {
	if (!h) return;
	{
		std::lock_guard<std::mutex> lk(h->mu);
		(void)hipSetDevice(h->device);
		if (h->stream) (void)hipStreamSynchronize(h->stream);
		for (int p = 1; p < polaris_hip_tracer::kMaxPipes; p++)
			if (h->pipe[p].q) (void)hipStreamSynchronize(h->pipe[p].q);
		if (h->fa.q) (void)hipStreamSynchronize(h->fa.q);
		collect_timers(h);
		std::lock_guard<std::mutex> lk_merge(h->fa.mu); // (a merge queued by another thread has left its critical section)
	}
	// The members release themselves, outside the locks (they are members too) and in no particular order.  Releasing "under the
	// locks and before the main stream goes", as this function once did by hand, was no constraint: a caller that destroys a handle
	// has no other call on it in flight, so the locks above only wait for one that is returning; and with every stream idle neither
	// hipFree nor the destruction of an event or stream depends on the main stream, or on each other.
	delete h;
}

const char *polaris_hip_last_error(polaris_hip_tracer *h) {
	if (!h) return g_thread_error.c_str();
	thread_local std::string copy; // a concurrent call may be failing on the same handle: read under the locks
	uint64_t seq;
	{
		std::lock_guard<std::mutex> lk(h->mu);
		copy = h->error;
		seq = h->error_seq;
	}
	{
		std::lock_guard<std::mutex> lk(h->fa.mu);
		if (h->fa.error_seq > seq) copy = h->fa.error; // the newer of the two
	}
	return copy.c_str();
}

int polaris_hip_resize(polaris_hip_tracer *h, uint32_t frame_w, uint32_t frame_h) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (frame_w == 0 || frame_h == 0 || (uint64_t)frame_w * frame_h > (1ull << 28))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "bad frame dimensions %ux%u", frame_w, frame_h);
	HIP_TRY(h, hipSetDevice(h->device));
	std::lock_guard<std::mutex> lk_merge(h->fa.mu); // (the frame accumulator is the merge stream's)
	HIP_TRY(h, sync_all(h));
	h->fa.release(); // everything of the old size goes before anything of the new size is allocated; no frame until all of it stands
	h->fs.resized();
	h->framebuffer.reset();
	const size_t F = (size_t)frame_w * frame_h;
	HIP_TRY(h, h->framebuffer.alloc(F));
	HIP_TRY(h, hipMemsetAsync(h->framebuffer, 0, F * sizeof(uchar4), h->stream));
	HIP_TRY(h, h->fa.resize(frame_w, frame_h, h->stream)); // (waits for the main stream)
	return POLARIS_OK;
}

int polaris_hip_upload_scene(polaris_hip_tracer *h, const PolarisSceneView *sc) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!sc) return fail(h, POLARIS_E_BAD_ARGUMENT, "scene view is null");
	SceneLayout L;
	if (int rc = layout_scene(h, *sc, L)) return rc; // 1. the layout: a refused scene changes nothing, the old one stays
	if (int rc = make_idle(h)) return rc;
	h->ds = DeviceScene(); // the old scene goes before the new one is allocated: a large one may not fit twice
	// 2. the history, judged by the instance table of the scene to come (kept with object motion only)
	InstTable next;
	if (h->fs.opt_object_motion) {
		next.num_triangles = sc->num_triangles;
		next.topology_known = true;
		next.mesh_index.resize(sc->num_mesh_instances);
		next.inv.resize((size_t)sc->num_mesh_instances * 16);
		for (uint32_t i = 0; i < sc->num_mesh_instances; i++) {
			next.mesh_index[i] = sc->mesh_instances[i].mesh_index;
			memcpy(next.inv.data() + 16 * (size_t)i, sc->mesh_instances[i].inv_transform, 16 * sizeof(float));
		}
	}
	h->fs.set_scene_deformable(h->opt_vertex_update != 0);
	h->fs.scene_changed(&next, h->camera.open);
	// 3. the arrays, with the triangle of every area light packed (shading.h, SceneT::light_geo); 4. what the updates keep
	std::vector<float> geo((size_t)sc->num_emissives * kLightGeoFloats, 0.0f);
	pack_light_geo(sc->emissives, sc->num_emissives, sc->vertices, sc->normals, sc->uvs, geo.data());
	int rc = upload_arrays(h, *sc, L, geo);
	if (!rc) rc = keep_update_plans(h, *sc, L, geo);
	if (!rc) rc = choose_traversal(h, *sc, L); // 5. how it is traversed
	if (rc) h->ds = DeviceScene(); // a failed upload leaves no scene, and no pointer to one
	else h->ds.have_scene = true;
	return rc;
}

// Move the uploaded scene's mesh instances in place (include/polaris_hip.h; instance_update.h has the arithmetic).
int polaris_hip_update_instances(polaris_hip_tracer *h, const PolarisInstanceUpdate *u) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	InstanceUpdateState &U = h->ds.upd;
	std::string msg;
	if (int st = check_instance_update(u, h->ds.have_scene, U.on, h->ds.num_insts, U.emissives, msg)) return fail(h, st, "%s", msg.c_str());
	const uint32_t NI = h->ds.num_insts;
	std::vector<InstUpdateRec> recs; std::vector<float> pads, geo;
	if (int st = prepare_instance_update(U.plan, NI, u->inv_transforms, u->instance_boxes, recs, pads, msg)) return fail(h, st, "%s", msg.c_str());
	if (u->emissives) { // the floats of the packed light records that depend on transform and area
		geo = U.light_geo;
		for (uint32_t e = 0; e < u->num_emissives; e++)
			if (u->emissives[e].type == POLARIS_EMISSIVE_AREA) derive_light_geo(u->emissives[e], geo.data() + (size_t)e * kLightGeoFloats);
	}
	// ---- accepted: from here on the state changes ----
	if (int rc = make_idle(h)) return rc;
	// to the temporal history the update is what an upload is: with object motion the planes synced under the old matrices join the
	// history, which stays -- instances and meshes are the same; without, the history saw the old scene and goes
	InstTable next = h->fs.v.cur;
	if (h->fs.opt_object_motion) next.inv.assign(u->inv_transforms, u->inv_transforms + (size_t)NI * 16);
	h->fs.scene_changed(&next, h->camera.open);
	if (h->ds.vup.on) h->ds.vup.inv.assign(u->inv_transforms, u->inv_transforms + (size_t)NI * 16);
	return finish_update(h, recs, pads, u->emissives, geo);
}

// Deform the uploaded scene's meshes in place (include/polaris_hip.h; vertex_update.h has the arithmetic).
int polaris_hip_update_vertices(polaris_hip_tracer *h, const PolarisVertexUpdate *u) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	InstanceUpdateState &U = h->ds.upd; VertexUpdateState &V = h->ds.vup;
	std::string msg;
	if (int st = check_vertex_update(u, h->ds.have_scene, V.on, U.plan.mesh, V.num_triangles, h->ds.num_insts, U.emissives, msg)) return fail(h, st, "%s", msg.c_str());
	const uint32_t NI = h->ds.num_insts;
	if (int st = check_vertex_magnitudes(u->vertices, V.num_triangles, msg)) return fail(h, st, "%s", msg.c_str());
	const float *inv = u->inv_transforms ? u->inv_transforms : V.inv.data();
	std::vector<InstUpdateRec> recs; std::vector<float> pads;
	// (matrices and boxes are judged now; the records and paddings are made again below, once the deformed meshes' boxes are known)
	if (int st = prepare_instance_update(U.plan, NI, inv, u->instance_boxes, recs, pads, msg)) return fail(h, st, "%s", msg.c_str());
	// the packed light records: the triangle of every area light from the new arrays (the uvs stay), then what derives from transform and area
	std::vector<float> geo = U.light_geo;
	pack_light_geo(u->emissives ? u->emissives : U.emissives.data(), U.emissives.size(), u->vertices, u->normals, nullptr, geo.data());
	// ---- accepted: from here on the state changes ----
	if (int rc = make_idle(h)) return rc;
	h->ds.have_scene = false; // (a failing call below leaves no scene, as a failed upload does)
	if (h->fs.features().deform_on()) {
		// with vertex motion in effect the update is to the history what update_instances is: the planes synced under the old vertices join
		// it and it stays -- topology, instances and meshes are the same -- and the vertices it was seen with are kept before they go
		InstTable next = h->fs.v.cur;
		if (u->inv_transforms) next.inv.assign(inv, inv + (size_t)NI * 16);
		h->fs.scene_changed(&next, h->camera.open);
		if (h->fs.v.vertices_changing(h->fs.features())) {
			const size_t nv = (size_t)V.num_triangles * 3;
			HIP_TRY(h, h->fs.vert_snap.reserve(nv)); // (the main stream is idle)
			HIP_TRY(h, hipMemcpyAsync(h->fs.vert_snap, V.vertices, nv * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
		}
	} else {
		h->fs.scene_changed(nullptr, h->camera.open); // the history never saw this scene
		if (h->fs.opt_object_motion && u->inv_transforms && h->fs.v.cur.inv.size() == (size_t)NI * 16) h->fs.v.cur.inv.assign(inv, inv + (size_t)NI * 16);
	}
	if (int rc = refit_meshes(h, u)) return rc;
	if (int st = prepare_instance_update(U.plan, NI, inv, u->instance_boxes, recs, pads, msg)) return fail(h, st, "%s", msg.c_str()); // (judged above: cannot fail)
	if (int rc = finish_update(h, recs, pads, u->emissives, geo)) return rc;
	if (u->inv_transforms) V.inv.assign(inv, inv + (size_t)NI * 16);
	h->ds.have_scene = true;
	return POLARIS_OK;
}

// Edit the uploaded scene's materials in place (include/polaris_hip.h; material_update.h has the arithmetic).
int polaris_hip_update_materials(polaris_hip_tracer *h, const PolarisMaterialUpdate *u) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	DeviceScene &S = h->ds;
	MaterialUpdateState &M = S.mup;
	std::string msg;
	if (int st = check_material_update(u, S.have_scene, S.scene.num_nodes, M.num_triangles, S.scene.num_emissives, S.scene.num_textures, msg)) return fail(h, st, "%s", msg.c_str());
	// what an upload derives from the node table: the class of every node, the classes that can end in an emitter
	std::vector<uint8_t> cls;
	const uint32_t emit_classes = classify_materials(u->material_nodes, u->num_material_nodes, S.scene.tri_bits, cls);
	// ---- accepted: from here on the state changes ----
	if (int rc = make_idle(h)) return rc;
	S.have_scene = false; // (a failing call below leaves no scene, as a failed upload does)
	h->fs.scene_changed(nullptr, h->camera.open); // the history never saw this scene
	hipStream_t q = h->stream;
	const uint32_t NE = u->emissive_mat_nodes ? S.scene.num_emissives : 0, cls_words = (uint32_t)(cls.size() / 4);
	HIP_TRY(h, h->d_retag.reserve((size_t)cls_words + NE + 4));
	HIP_TRY(h, hipMemcpyAsync(M.nodes, u->material_nodes, (size_t)u->num_material_nodes * sizeof(PolarisMaterialNode), hipMemcpyHostToDevice, q));
	HIP_TRY(h, hipMemcpyAsync(h->d_retag, cls.data(), cls.size(), hipMemcpyHostToDevice, q));
	if (u->material_index) HIP_TRY(h, hipMemcpyAsync(M.mat_index, u->material_index, (size_t)M.num_triangles * sizeof(uint32_t), hipMemcpyHostToDevice, q));
	if (NE) {
		HIP_TRY(h, hipMemcpyAsync(h->d_retag + cls_words, u->emissive_mat_nodes, (size_t)NE * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		(void)launch(h, nullptr, q, kEmissiveNodes, (NE + kRetagBlock - 1) / kRetagBlock, kRetagBlock, 0, M.emissives, h->d_retag + cls_words, NE);
	}
	if (S.scene.tri_bits < 31) { // (else hits carry no class: nothing to retag, emit_classes stays all ones)
		const uint32_t per_group = kRetagBlock * kRetagSlotsPerThread;
		(void)launch(h, "retag", q, kRetag, (M.num_slots + per_group - 1) / per_group, kRetagBlock, 0, M.tris, M.num_slots, M.mat_index,
		             reinterpret_cast<const uint8_t *>(h->d_retag.get()), u->num_material_nodes, S.scene.tri_bits, M.meta_word ? 1u : 0u);
	}
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipStreamSynchronize(q)); // (the caller's arrays and cls may go at return)
	collect_timers(h);
	S.scene.bg_node = u->scene_diffuse_mat_index;
	S.scene.emit_classes = emit_classes; // (every Trace plans from it anew: plan_scene)
	// the host copy of the emissive list the other two updates judge and re-send follows, or they would refuse the new list or revert the field
	for (uint32_t e = 0; e < NE && e < S.upd.emissives.size(); e++) S.upd.emissives[e].mat_node_index = u->emissive_mat_nodes[e];
	S.have_scene = true;
	return POLARIS_OK;
}

int polaris_hip_update_texture(polaris_hip_tracer *h, uint32_t index, const void *texels, size_t n_bytes) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	DeviceScene &S = h->ds;
	std::string msg;
	if (int st = check_texture_update(index, texels, n_bytes, S.have_scene, S.mup.tex_meta, msg)) return fail(h, st, "%s", msg.c_str());
	if (int rc = make_idle(h)) return rc;
	S.have_scene = false;
	h->fs.scene_changed(nullptr, h->camera.open);
	if (n_bytes) HIP_TRY(h, hipMemcpyAsync(S.mup.tex_data + S.mup.tex_meta[index].data_offset, texels, n_bytes, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	S.have_scene = true;
	return POLARIS_OK;
}

int polaris_hip_read_scene_records(polaris_hip_tracer *h, int which, void *out, size_t n_bytes) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
	if (which < POLARIS_REC_PAIRS || which > POLARIS_REC_SHADING) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_scene_records: unknown record kind %d", which);
	uint64_t counts[4] = {h->ds.bvh.num_pairs, h->ds.num_insts, h->ds.bufs.size(), 0};
	for (const DevArray<char> &b : h->ds.bufs) counts[3] += b.capacity();
	const uint32_t shading[4] = {h->ds.scene.tri_bits, h->ds.scene.emit_classes, (uint32_t)h->ds.scene.bg_node, h->ds.mup.num_slots};
	const size_t need = which == POLARIS_REC_COUNTS ? sizeof counts : which == POLARIS_REC_SHADING ? sizeof shading :
	                    which == POLARIS_REC_TRIS ? (size_t)h->ds.mup.num_slots * sizeof(TriRec) : (size_t)counts[which] * 64;
	if (!out || n_bytes < need) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_scene_records: need %zu bytes", need);
	if (which == POLARIS_REC_COUNTS) { memcpy(out, counts, sizeof counts); return POLARIS_OK; }
	if (which == POLARIS_REC_SHADING) { memcpy(out, shading, sizeof shading); return POLARIS_OK; }
	HIP_TRY(h, hipSetDevice(h->device));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	const void *src = which == POLARIS_REC_PAIRS ? (const void *)h->ds.bvh.pairs : which == POLARIS_REC_INSTS ? (const void *)h->ds.bvh.insts : (const void *)h->ds.bvh.tris;
	HIP_TRY(h, hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
	return POLARIS_OK;
}

// What the three camera setters share: perform what the transition asks (camera_state.h CameraTodo) and commit its state, or
// report its refusal; a step that fails here leaves the camera as it was.  The caller holds mu.  eye: polaris_hip_set_camera's.
static int apply_camera_step(polaris_hip_tracer *h, const CameraStep &s, const float *eye = nullptr) {
	if (!s.refusal.empty()) return fail(h, POLARIS_E_BAD_ARGUMENT, "%s", s.refusal.c_str());
	const bool drop = (s.todo & kCamDropHistory) && h->fs.tp.max_history;
	const bool projection = (s.todo & kCamProjection) != 0;
	if (drop || eye || projection) HIP_TRY(h, hipSetDevice(h->device));
	if (drop || projection) HIP_TRY(h, hipStreamSynchronize(h->stream)); // the history's planes are freed: the main stream, where every temporal launch runs, is idle first
	if (eye) { // the one origin record of every camera ray: what k_generate would write per ray (kernels.h)
		const float4 o4 = make_float4(eye[0], eye[1], eye[2], kFltMax);
		// (nothing of this handle reads the record now: the caller holds mu, and a Trace returns only when its kernels are done)
		HIP_TRY(h, hipMemcpy(h->d_cam_o, &o4, sizeof o4, hipMemcpyHostToDevice));
	}
	if (drop) h->fs.lens_changed();
	if (projection) h->fs.projection_changed();
	if (s.todo & kCamMoved) h->fs.camera_moved(h->camera.open); // (with temporal reuse the last temporal sync's planes under the old camera become the history)
	h->camera = s.next;
	return POLARIS_OK;
}

int polaris_hip_set_camera(polaris_hip_tracer *h, const float eye[3], const float fr[16]) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	return apply_camera_step(h, h->camera.set_camera(eye, fr), eye);
}

int polaris_hip_set_lens(polaris_hip_tracer *h, const PolarisLensParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	return apply_camera_step(h, h->camera.set_lens(p));
}

int polaris_hip_set_shutter(polaris_hip_tracer *h, const PolarisShutterParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	return apply_camera_step(h, h->camera.set_shutter(p));
}

int polaris_hip_set_projection(polaris_hip_tracer *h, const PolarisProjectionParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	return apply_camera_step(h, h->camera.set_projection(p));
}

int polaris_hip_set_option(polaris_hip_tracer *h, const char *key, int64_t value) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!key) return fail(h, POLARIS_E_BAD_ARGUMENT, "option key is null");
	const std::string k(key);
	if (k == "samples_per_batch") h->opt.samples_per_batch = value < 0 ? 0 : value;
	else if (k == "exact_accumulate") {
		if (value != 0 && h->opt_moments) return fail(h, POLARIS_E_UNSUPPORTED, "exact_accumulate has no per-sample radiance: it cannot be combined with moments");
		h->opt.exact = value != 0;
	} else if (k == "moments") {
		if (value != 0 && h->opt.exact) return fail(h, POLARIS_E_UNSUPPORTED, "moments need per-sample radiance: exact_accumulate cannot keep them");
		if (value == 0 && h->fs.va.sigma_variance != 0.0f) return fail(h, POLARIS_E_BAD_ARGUMENT, "moments cannot be turned off while variance guidance is on");
		h->opt_moments = value != 0;
	}
	else if (k == "packet_primary") { h->opt.packet_primary = value < 0 ? -1 : (value != 0); if (value >= 0) h->packet_primary = value != 0; }
	else if (k == "packet_shadow") h->opt.packet_shadow = (int)std::max<int64_t>(0, std::min<int64_t>(value, POLARIS_MAX_BOUNCES));
	else if (k == "time_kernels") h->opt_time_kernels = value != 0;
	else if (k == "node_mode") h->opt_node_mode = (int)std::max<int64_t>(-1, std::min<int64_t>(value, 2)); // next upload; 2 only where the scene is tiny enough
	else if (k == "traversal") h->opt.traversal = value != 0; // 0 = one ray per lane (k_intersect / k_occlusion), 1 = persistent waves with lane refill (k_trace)
	else if (k == "shade_wave") h->opt.shade_wave = value != 0;
	else if (k == "shade_wave_from") h->opt.shade_wave_from = (int)std::max<int64_t>(-1, std::min<int64_t>(value, POLARIS_MAX_BOUNCES));
	else if (k == "shade_wgs_per_cu") h->opt.shade_wgs_per_cu = (int)std::max<int64_t>(0, std::min<int64_t>(value, 64));
	else if (k == "stage_lds") h->opt.stage_lds = value != 0;
	else if (k == "shade_prefilter") h->opt.shade_prefilter = value != 0;
	else if (k == "shade_sort") h->opt.shade_sort = (int)std::max<int64_t>(-1, std::min<int64_t>(value, POLARIS_MAX_BOUNCES));
	else if (k == "ipc_staged") h->fa.ipc_staged = value != 0;
	else if (k == "overlap") h->opt.overlap = (int)std::max<int64_t>(1, std::min<int64_t>(value, polaris_hip_tracer::kMaxPipes));
	else if (k == "trace_grid") h->opt.trace_grid = (int)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 20));
	else if (k == "trace_wgs_per_cu") h->opt.trace_wgs_per_cu = (int)std::max<int64_t>(0, std::min<int64_t>(value, 64));
	else if (k == "tiny_one") h->opt_tiny_one = value != 0; // next upload
	else if (k == "hit12") h->opt.hit12 = value != 0;
	else if (k == "o12") h->opt.o12 = value != 0;
	else if (k == "lds_tris") h->opt_lds_tris = (int)std::max<int64_t>(-1, std::min<int64_t>(value, 1 << 20)); // next upload
	else if (k == "object_motion") {
		if (value != 0 && value != 1) return fail(h, POLARIS_E_BAD_ARGUMENT, "object_motion is 0 or 1");
		if ((int)value != h->fs.opt_object_motion) {
			HIP_TRY(h, hipSetDevice(h->device));
			HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every launch that uses the planes that go is on the main stream)
			h->fs.set_object_motion((int)value);
			if (value && h->ds.have_scene)
				if (int rc = read_back_instances(h)) return rc;
		}
	}
	else if (k == "vertex_motion") {
		if (value != 0 && value != 1) return fail(h, POLARIS_E_BAD_ARGUMENT, "vertex_motion is 0 or 1");
		if ((int)value != h->fs.opt_vertex_motion) {
			HIP_TRY(h, hipSetDevice(h->device));
			HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every launch that uses the planes that go is on the main stream)
			h->fs.set_vertex_motion((int)value);
		}
	}
	else if (k == "bloom_fused") { // an A/B switch, the pyramid's values do not depend on it
		if (value != 0 && value != 1) return fail(h, POLARIS_E_BAD_ARGUMENT, "bloom_fused is 0 or 1");
		h->fs.bl.fused = (int)value;
	}
	else if (k == "guide_specular") {
		if (value < 0 || value > 8) return fail(h, POLARIS_E_BAD_ARGUMENT, "guide_specular is 0..8");
		if ((int)value != h->fs.opt_guide_specular) h->fs.set_guide_specular((int)value); // (no plane is freed: nothing to wait for)
	}
	else if (k == "instance_update") { // next upload
		if (value != 0 && value != 1) return fail(h, POLARIS_E_BAD_ARGUMENT, "instance_update is 0 or 1");
		h->opt_instance_update = (int)value;
	}
	else if (k == "vertex_update") { // next upload
		if (value != 0 && value != 1) return fail(h, POLARIS_E_BAD_ARGUMENT, "vertex_update is 0 or 1");
		h->opt_vertex_update = (int)value;
	}
	else if (k == "max_leaf_tris") h->opt_max_leaf_tris = (int)std::max<int64_t>(-1, std::min<int64_t>(value, 1 << 20)); // next upload
	else return fail(h, POLARIS_E_BAD_ARGUMENT, "unknown option '%s'", key);
	return POLARIS_OK;
}

int polaris_hip_trace(polaris_hip_tracer *h, const PolarisBlockRequest *r, const uint32_t *seeds, size_t n_seeds,
                      PolarisTraceStats *stats) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	// a Trace that resets the frame announces it (reset epoch) once the clear is queued -- or when it fails before that, so
	// that nobody waits for a reset that will not come
	struct ResetAnnounce {
		FrameAccum &fa; bool due;
		~ResetAnnounce() { if (due) (void)fa.reset_frame(false); }
	} announce{h->fa, r && r->accumulated_samples == 0};
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded"); // ErrNoSceneData, tracer.go:203-205
	if (int rc = check_request(h, r)) return rc;
	if (!h->camera.have_camera) return fail(h, POLARIS_E_BAD_ARGUMENT, "camera not set (UpdateState CameraData)");
	const uint32_t B = r->num_bounces, spp = r->samples_per_pixel;
	if (B > POLARIS_MAX_BOUNCES) return fail(h, POLARIS_E_BAD_ARGUMENT, "num_bounces %u exceeds %d", B, POLARIS_MAX_BOUNCES);
	const size_t need_seeds = (size_t)spp * (1 + B);
	if (need_seeds && (!seeds || n_seeds < need_seeds))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "seed list has %zu entries, need samples*(1+bounces) = %zu", n_seeds, need_seeds);
	const uint64_t N64 = (uint64_t)h->fa.W * r->block_h;
	if (N64 > (1u << 24)) // the reference stores the path index as a float in ray.dir.w (util/ray.cl:9-12)
		return fail(h, POLARIS_E_BAD_ARGUMENT, "block has %llu pixels; the path index is exact only below 2^24", (unsigned long long)N64);
	const uint32_t N = (uint32_t)N64, Npad = (N + WG - 1) / WG * WG;

	HIP_TRY(h, hipSetDevice(h->device));
	// plan (trace_plan.h): the batch size, clamped by the free device memory where the plan chose it itself
	TracePlan plan = plan_trace(h->opt, plan_scene(h), h->opt_moments, spp, B, r->min_bounces_for_rr, Npad);
	size_t free_b = 0, total_b = 0;
	if (plan.wants_memory_clamp() && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
		size_t have = 0; // what the pipelines already hold counts as available
		for (auto &P : h->pipe) have += P.slots * slot_bytes(P.nee_bounces);
		plan.clamp_to_memory(free_b + have);
	}
	// allocate: an allocation that fails for want of memory releases every pipeline's buffers and asks the plan for the next smaller batch
	for (;;) {
		int rc = POLARIS_OK;
		for (int p = 0; p < plan.n_pipes && rc == POLARIS_OK; p++) rc = ensure_streams(h, p, (size_t)plan.K * Npad, false, plan.exact ? 1u : B);
		if (rc == POLARIS_OK) break;
		if (!plan.shrink()) return rc;
		(void)hipGetLastError();
		for (auto &P : h->pipe)
			if (P.q && P.slots) { (void)hipStreamSynchronize(P.q); P.release(); }
	}
	const uint32_t K = plan.K;
	const int n_pipes = plan.n_pipes;
	HIP_TRY(h, h->d_seeds.reserve(need_seeds));
	const size_t F = (size_t)h->fa.W * h->fa.H;
	hipStream_t q = h->stream;
	// The next slot of the ring: a peer may still be reading the previous frame's rows (polaris_hip_ipc_export).  Advanced only
	// HERE, behind the last step that can fail for want of memory (the batch buffers, the seed list): after a Trace that failed
	// before it queued anything, trace_slot() / merge_slot / export_block still name the slot of the last frame that was traced.
	h->fa.advance();
	HIP_TRY(h, hipEventRecord(h->ev_start, q));
	if (announce.due) { // pipeline Reset stage (tracer.go:208-213): the frame accumulator lives on the merge stream
		announce.due = false;
		HIP_TRY(h, h->fa.reset_frame()); // merges queued from here on land on the cleared accumulator
	}
	// A merge that still READS this tracer's trace accumulator (MergeOutput(self) runs on the merge stream; Trace -> MergeOutput(self)
	// -> Trace without a SyncFramebuffer in between is the progressive loop) must be done before the rows are cleared and
	// rewritten: a device-side wait, the host does not block.  (A merge queued by ANOTHER handle onto its own merge stream
	// -- dst != src -- is ordered by the peer-read fence in polaris_hip_merge: src's `readers` event, below.)
	HIP_TRY(h, h->fa.join_merges(q));
	HIP_TRY(h, h->fa.wait_readers(q));
	HIP_TRY(h, hipMemsetAsync(h->fa.current(), 0, F * sizeof(float4), q)); // ClearTraceAccumulator (tracer.go:215)
	HIP_TRY(h, hipMemsetAsync(h->d_stats, 0, ST_COUNT * sizeof(unsigned long long), q));
	if (need_seeds) HIP_TRY(h, hipMemcpyAsync(h->d_seeds, seeds, need_seeds * sizeof(uint32_t), hipMemcpyHostToDevice, q));
	if (n_pipes > 1) { // fork: the other pipelines start after the clears and the seed upload
		HIP_TRY(h, hipEventRecord(h->ev_fork, q));
		for (int p = 1; p < n_pipes; p++) HIP_TRY(h, hipStreamWaitEvent(h->pipe[p].q, h->ev_fork, 0));
	}
	// From here on batches are in flight on several streams: a failure must not return before every one
	// of them has drained (resize / upload_scene / destroy free what the kernels still write to).
	struct DrainOnError {
		polaris_hip_tracer *h; int n; bool armed = true;
		~DrainOnError() { if (armed) for (int p = 0; p < n; p++) (void)hipStreamSynchronize(h->pipe[p].q); }
	} drain{h, n_pipes};
	for (uint32_t b = 0; b < B && spp; b++) h->last_shade_timer[b] = plan.bounce[b].shade;
	uint32_t bi = 0;
	for (uint32_t s0 = 0; s0 < spp; s0 += K, bi++) {
		const int p = (int)(bi % (uint32_t)n_pipes), prev = (int)((bi + (uint32_t)n_pipes - 1) % (uint32_t)n_pipes);
		HIP_TRY(h, launch_batch(h, p, r, plan, s0, std::min(K, spp - s0), N, (n_pipes > 1 && bi > 0) ? h->pipe[prev].done : nullptr));
	}
	for (int p = 1; p < n_pipes; p++) HIP_TRY(h, hipStreamWaitEvent(q, h->pipe[p].done, 0)); // join
	HIP_TRY(h, hipGetLastError());
	unsigned long long hs[ST_COUNT];
	HIP_TRY(h, hipMemcpyAsync(hs, h->d_stats, sizeof hs, hipMemcpyDeviceToHost, q));
	if (hipEvent_t done = h->fa.ev_done[h->fa.ix.pos]) HIP_TRY(h, hipEventRecord(done, q)); // what a peer process's merge of THIS slot waits for (polaris_hip_merge_ipc)
	HIP_TRY(h, hipEventRecord(h->ev_stop, q));
	HIP_TRY(h, hipStreamSynchronize(q));
	drain.armed = false; // the join above made q wait for every pipeline
	collect_timers(h);
	for (uint32_t b = 0; b < POLARIS_MAX_BOUNCES; b++) {
		h->last_shade_counts[3 * b] = b < B ? hs[ST_HITS_BOUNCE + b] : 0;
		h->last_shade_counts[3 * b + 1] = b < B ? hs[ST_MISSES_BOUNCE + b] : 0;
		h->last_shade_counts[3 * b + 2] = b < B ? hs[ST_EMITTERS_BOUNCE + b] : 0;
	}
	if (stats) {
		memset(stats, 0, sizeof *stats);
		stats->primary_rays = (uint64_t)N * spp;
		for (uint32_t b = 0; b < B; b++) {
			stats->shaded_hits += hs[ST_HITS_BOUNCE + b];
			stats->shaded_misses += hs[ST_MISSES_BOUNCE + b];
			stats->emitter_hits += hs[ST_EMITTERS_BOUNCE + b];
		}
		stats->unoccluded = hs[ST_UNOCCLUDED];
		if (B > 0) stats->rays_per_bounce[0] = (uint64_t)N * spp;
		for (uint32_t b = 1; b < B; b++) {
			stats->rays_per_bounce[b] = hs[ST_RAYS_BOUNCE + b];
			stats->indirect_rays += hs[ST_RAYS_BOUNCE + b];
		}
		for (uint32_t b = 0; b < B; b++) {
			stats->occl_per_bounce[b] = hs[ST_OCCL_BOUNCE + b];
			stats->occlusion_rays += hs[ST_OCCL_BOUNCE + b];
		}
		float ms = 0.0f;
		(void)hipEventElapsedTime(&ms, h->ev_start, h->ev_stop);
		stats->device_ms = ms;
	}
	return POLARIS_OK;
}

// What a MergeOutput reads: one slot of a trace accumulator ring, resolved by the entry point that names it.
struct MergeSource {
	MergeKind kind = MergeKind::SameDevice;
	const float4 *acc = nullptr; // the slot, from its first row on (null: the source has no frame)
	uint32_t W = 0, H = 0;
	int device = 0, slot = -1;         // the GPU it lies on (a peer's: dst's, where it is mapped) | a peer's slot
	polaris_hip_tracer *src = nullptr; // a tracer of this process: fenced against its next Trace
	polaris_hip_peer *peer = nullptr;  // another process's ring
	const char *refusal = nullptr;     // why there is nothing to read
};

// A tracer of this process (polaris_hip_merge: slot < 0, its current slot; polaris_hip_merge_slot).  Its trace accumulator is complete
// (its Trace is synchronous and has returned): snapshot what is needed of it under ITS lock, briefly, and before dst's merge lock.
static MergeSource tracer_source(const polaris_hip_tracer *dst, polaris_hip_tracer *src, int slot) {
	MergeSource S;
	std::lock_guard<std::mutex> lk_src(src->mu);
	S.src = src; S.device = src->device; S.W = src->fa.W; S.H = src->fa.H;
	S.kind = S.device == dst->device ? MergeKind::SameDevice : MergeKind::OtherDevice;
	S.acc = src->fa.slot(slot);
	if (src->fa.ix.slot_of(slot) < 0) S.refusal = "merge: ring slot out of range";
	return S;
}

// Another process's ring, mapped on dst's device (polaris_hip_merge_ipc; caller holds dst->fa.mu).
static MergeSource peer_source(const polaris_hip_tracer *dst, polaris_hip_peer *peer, int slot) {
	MergeSource S;
	S.kind = MergeKind::PeerRing; S.peer = peer; S.slot = slot; S.device = dst->device; S.W = peer->W; S.H = peer->H;
	if (peer->owner != dst) S.refusal = "merge_ipc: the peer was opened by another tracer";
	else if ((uint32_t)slot >= peer->depth) S.refusal = "merge: ring slot out of range";
	else S.acc = (const float4 *)peer->mem[slot].get();
	return S;
}

// MergeOutput: the block's rows of S onto dst's frame accumulator.  Everything on dst's merge stream, under dst->fa.mu (which the
// caller holds) only -- never under dst->mu, which the destination's own Trace holds from start to end.
static int merge_rows(polaris_hip_tracer *dst, const MergeSource &S, const PolarisBlockRequest *r) {
	FrameAccum &A = dst->fa;
	if (S.refusal) return A.fail(POLARIS_E_BAD_ARGUMENT, S.refusal);
	switch (const BlockRefusal why = refuse_block(A.W, A.H, r)) {
	case BlockRefusal::None: break;
	case BlockRefusal::FrameMismatch: return A.fail(POLARIS_E_BAD_ARGUMENT, "merge: request frame does not match the tracer's");
	case BlockRefusal::RowsOutside: return A.fail(POLARIS_E_BAD_ARGUMENT, "merge: block rows outside the frame");
	default: return A.fail(POLARIS_E_BAD_ARGUMENT, kBlockRefusal[(int)why]);
	}
	if (S.W != A.W || S.H != A.H || !S.acc) return A.fail(POLARIS_E_BAD_ARGUMENT, "merge: source tracer has different frame dimensions");
	if (hipSetDevice(dst->device) != hipSuccess) return A.fail(POLARIS_E_DEVICE, "merge: hipSetDevice failed");
	const size_t off = (size_t)r->block_y * A.W, n = (size_t)r->block_h * A.W;
	const float4 *rows = S.acc + off;
	if (S.peer && S.peer->ev[S.slot] && hipStreamWaitEvent(A.q, S.peer->ev[S.slot], 0) != hipSuccess) {
		// The device-side wait is belt and braces: the slot was announced by a host message AFTER the peer's synchronous Trace returned, so
		// its rows are complete.  A runtime that refuses to wait for another process's / another device's event must not cost the frame:
		// drop the peer's events (the wait is not retried) and go on with the host-side ordering alone.
		(void)hipGetLastError();
		S.peer->drop_events();
		(void)hipGetLastError();
		if (getenv("POLARIS_DEBUG")) fprintf(stderr, "[polaris] merge_ipc: hipStreamWaitEvent on the peer's inter-process event failed; continuing with the host-side ordering\n");
	}
	// the route (merge_plan.h): another GPU of this process is read in place only with peer access, asked for here
	int can = -1;
	bool enabled = false;
	if (S.kind == MergeKind::OtherDevice) {
		if (hipDeviceCanAccessPeer(&can, dst->device, S.device) != hipSuccess) can = -1;
		else if (can) {
			const hipError_t e = hipDeviceEnablePeerAccess(S.device, 0);
			can = 1;
			enabled = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
			(void)hipGetLastError();
		}
	}
	const PolarisPeerInfo *I = S.peer ? &S.peer->info : nullptr;
	const MergeRoute route = route_merge(S.kind, I ? I->same_device : -1, I && I->staged, can, enabled);
	if (route.branch < 0) return A.fail(POLARIS_E_DEVICE, "merge: hipDeviceCanAccessPeer failed");
	if (route.rows != RowsTravel::InPlace) { // the RUNTIME moves the rows into the staging strip, the kernel adds a local strip
		if (!A.need_staging(n)) return A.fail(POLARIS_E_DEVICE, "merge: out of device memory for the staging strip");
		if (route.rows == RowsTravel::DefaultCopy) {
			if (hipMemcpyAsync(A.staging, rows, n * sizeof(float4), hipMemcpyDefault, A.q) != hipSuccess) return A.fail(POLARIS_E_DEVICE, "merge_ipc: hipMemcpyAsync from the peer's ring failed");
		} else if (hipMemcpyPeerAsync(A.staging, dst->device, rows, S.device, n * sizeof(float4), A.q) != hipSuccess) return A.fail(POLARIS_E_DEVICE, "merge: hipMemcpyPeerAsync failed");
		rows = A.staging;
	}
	hipError_t launched;
	{
		Timed t(dst, "aggregate", nullptr, A.q, true);
		launched = A.add_rows(rows, off, n, dst->opt_moments, route.branch);
	}
	if (launched != hipSuccess) return A.fail(POLARIS_E_DEVICE, "merge: kernel launch failed");
	// src's next Trace clears and rewrites the rows just queued for reading: it waits (on the device) for this event.  With
	// src == dst the merge stream itself is joined by Trace (join_merges).  Recorded for a merge from a named ring slot too
	// (merge_slot): with a ring of depth 1 that slot IS what the next Trace clears, and with a deeper ring the wait is for a
	// kernel of microseconds.
	if (S.src && S.src != dst) {
		DevEvent e = S.src->fa.reader_event(dst->device);
		if (!e || hipEventRecord(e, A.q) != hipSuccess) { // cannot fence on the device: finish the read now
			(void)hipGetLastError();
			if (hipStreamSynchronize(A.q) != hipSuccess) return A.fail(POLARIS_E_DEVICE, "merge: hipStreamSynchronize failed");
		} else S.src->fa.add_reader(std::move(e), dst->device);
	}
	return POLARIS_OK; // asynchronous like Exec1DNoWait (resources.go:119); completed by sync_framebuffer
}

int polaris_hip_merge(polaris_hip_tracer *dst, polaris_hip_tracer *src, const PolarisBlockRequest *r) {
	if (!dst || !src) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge: null tracer handle");
	const MergeSource S = tracer_source(dst, src, -1);
	std::lock_guard<std::mutex> lk(dst->fa.mu);
	return merge_rows(dst, S, r);
}

int polaris_hip_merge_slot(polaris_hip_tracer *dst, polaris_hip_tracer *src, uint32_t slot, const PolarisBlockRequest *r) {
	if (!dst || !src) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge_slot: null tracer handle");
	if (slot >= POLARIS_IPC_MAX_DEPTH) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge_slot: ring slot out of range");
	const MergeSource S = tracer_source(dst, src, (int)slot);
	std::lock_guard<std::mutex> lk(dst->fa.mu);
	return merge_rows(dst, S, r);
}

int polaris_hip_merge_ipc(polaris_hip_tracer *dst, polaris_hip_peer *peer, uint32_t slot, const PolarisBlockRequest *r) {
	if (!dst || !peer) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge_ipc: null handle");
	if (slot >= POLARIS_IPC_MAX_DEPTH) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge_ipc: ring slot out of range");
	std::lock_guard<std::mutex> lk(dst->fa.mu);
	return merge_rows(dst, peer_source(dst, peer, (int)slot), r);
}

int polaris_hip_trace_slot(polaris_hip_tracer *h, uint32_t *slot) {
	if (!h || !slot) return fail(h, POLARIS_E_BAD_ARGUMENT, "trace_slot: null argument");
	std::lock_guard<std::mutex> lk(h->mu);
	*slot = h->fa.ix.pos;
	return POLARIS_OK;
}

// The trace accumulator becomes a ring of `depth` IPC-exportable buffers; `out` = what a peer process needs to map them.
int polaris_hip_ipc_export(polaris_hip_tracer *h, uint32_t depth, PolarisIpcExport *out) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!out) return fail(h, POLARIS_E_BAD_ARGUMENT, "ipc_export: out is null");
	if (depth < 1 || depth > POLARIS_IPC_MAX_DEPTH) return fail(h, POLARIS_E_BAD_ARGUMENT, "ipc_export: depth must be 1..%d", POLARIS_IPC_MAX_DEPTH);
	if (h->fa.W == 0 || h->fa.H == 0 || !h->fa.ring[0]) return fail(h, POLARIS_E_BAD_ARGUMENT, "frame dimensions not set (UpdateState FrameDimensions)");
	static_assert(sizeof(hipIpcMemHandle_t) == 64 && sizeof(hipIpcEventHandle_t) == 64, "PolarisIpcExport holds 64-byte handles");
	HIP_TRY(h, hipSetDevice(h->device));
	std::lock_guard<std::mutex> lk_merge(h->fa.mu);
	HIP_TRY(h, sync_all(h));
	HIP_TRY(h, h->fa.redepth(depth, h->stream));
	memset(out, 0, sizeof *out);
	out->abi_version = POLARIS_HIP_ABI_VERSION; out->depth = depth; out->frame_w = h->fa.W; out->frame_h = h->fa.H;
	out->device = h->device; out->pid = (uint32_t)getpid();
	static_assert(sizeof out->pci_bus_id == sizeof h->pci_bus_id, "the export carries the tracer's bus id as it is");
	memcpy(out->pci_bus_id, h->pci_bus_id, sizeof out->pci_bus_id);
	for (uint32_t i = 0; i < depth; i++) {
		hipIpcMemHandle_t mh;
		HIP_TRY(h, hipIpcGetMemHandle(&mh, h->fa.ring[i]));
		memcpy(out->mem[i], &mh, 64);
	}
	// the per-slot "Trace done" events: optional (a runtime that cannot export events still has the host-side ordering: Trace is
	// synchronous, and a slot is only announced after the Trace that wrote it has returned).  All slots or none.
	bool events = true;
	for (uint32_t i = 0; i < depth; i++) { // (redepth dropped the events of the slots that went)
		DevEvent &done = h->fa.ev_done[i];
		if (!done && done.create(hipEventCreateWithFlags, hipEventDisableTiming | hipEventInterprocess) != hipSuccess) {
			(void)hipGetLastError(); events = false; break;
		}
		hipIpcEventHandle_t eh;
		if (hipEventRecord(done, h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess &&
		    hipIpcGetEventHandle(&eh, done) == hipSuccess) memcpy(out->event[i], &eh, 64);
		else { (void)hipGetLastError(); events = false; break; }
	}
	if (!events) {
		for (auto &e : h->fa.ev_done) e.reset();
		memset(out->event, 0, sizeof out->event);
	}
	out->has_event = events ? 1 : 0;
	return POLARIS_OK;
}

int polaris_hip_ipc_open(polaris_hip_tracer *dst, const PolarisIpcExport *x, polaris_hip_peer **out) {
	if (!dst) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(dst->mu);
	if (!x || !out) return fail(dst, POLARIS_E_BAD_ARGUMENT, "ipc_open: null argument");
	*out = nullptr;
	if (x->abi_version != POLARIS_HIP_ABI_VERSION) return fail(dst, POLARIS_E_BAD_ARGUMENT, "ipc_open: the export was made by ABI version %u, this library is %d", x->abi_version, POLARIS_HIP_ABI_VERSION);
	if (x->depth < 1 || x->depth > POLARIS_IPC_MAX_DEPTH) return fail(dst, POLARIS_E_BAD_ARGUMENT, "ipc_open: bad ring depth %u", x->depth);
	if (x->frame_w != dst->fa.W || x->frame_h != dst->fa.H || dst->fa.W == 0) return fail(dst, POLARIS_E_BAD_ARGUMENT, "ipc_open: the peer's frame %ux%u does not match the tracer's %ux%u", x->frame_w, x->frame_h, dst->fa.W, dst->fa.H);
	if (x->pid == (uint32_t)getpid()) return fail(dst, POLARIS_E_UNSUPPORTED, "ipc_open: the export comes from this process (HIP cannot open its own IPC handle): use polaris_hip_merge / polaris_hip_merge_slot");
	HIP_TRY(dst, hipSetDevice(dst->device));
	std::unique_ptr<polaris_hip_peer> p(new polaris_hip_peer()); // (a failure below closes what was opened)
	p->owner = dst; p->depth = x->depth; p->W = x->frame_w; p->H = x->frame_h;
	{ // what the mapping is: the exporter's GPU by bus id, as this process sees it
		PolarisPeerInfo &I = p->info;
		I.struct_size = sizeof I; I.pid = x->pid; I.exporter_device = x->device;
		I.depth = x->depth;
		memcpy(I.pci_bus_id, x->pci_bus_id, sizeof I.pci_bus_id);
		I.pci_bus_id[sizeof I.pci_bus_id - 1] = 0;
		// the runtime's answers; merge_plan.h classify_peer decides what they mean
		const bool have_ids = I.pci_bus_id[0] && dst->pci_bus_id[0], same_id = have_ids && strcmp(I.pci_bus_id, dst->pci_bus_id) == 0;
		int local = -1, can = -1;
		if (have_ids && hipDeviceGetByPCIBusId(&local, I.pci_bus_id) != hipSuccess) { (void)hipGetLastError(); local = -1; }
		if (have_ids && !same_id && local >= 0 && local != dst->device && hipDeviceCanAccessPeer(&can, dst->device, local) != hipSuccess) { (void)hipGetLastError(); can = -1; }
		const PeerClass c = classify_peer(have_ids, same_id, dst->device, local, can, dst->fa.ipc_staged != 0);
		I.same_device = c.same_device; I.local_device = c.local_device; I.can_access_peer = c.can_access_peer; I.staged = c.staged;
		if (!c.visible) { // (a per-rank visibility mask: the caller has its strip fallback)
			return fail(dst, POLARIS_E_UNSUPPORTED, "ipc_open: the peer's ring lives on GPU %s, which is not visible to this process (device visibility mask?): "
			            "a peer mapping cannot be verified; use a transport that does not need one", I.pci_bus_id);
		}
	}
	for (uint32_t i = 0; i < x->depth; i++) {
		hipIpcMemHandle_t mh;
		memcpy(&mh, x->mem[i], 64);
		const hipError_t e = p->mem[i].create(hipIpcOpenMemHandle, mh, hipIpcMemLazyEnablePeerAccess);
		if (e != hipSuccess) {
			p.reset();
			(void)hipGetLastError();
			return fail(dst, POLARIS_E_UNSUPPORTED, "ipc_open: hipIpcOpenMemHandle (slot %u, peer pid %u device %d): %s", i, x->pid, x->device, hipGetErrorString(e));
		}
	}
	if (x->has_event) { // optional: without them the host message that follows the peer's synchronous Trace is the only ordering
		for (uint32_t i = 0; i < x->depth; i++) {
			hipIpcEventHandle_t eh;
			memcpy(&eh, x->event[i], 64);
			if (p->ev[i].create(hipIpcOpenEventHandle, eh) != hipSuccess) { // all or none
				(void)hipGetLastError();
				p->drop_events();
				break;
			}
		}
	}
	// Every slot's event was recorded (and waited for) once by the export, so each must read COMPLETE here.  One that does not -- its state
	// is not visible in this process (another device, another container) -- would make a merge's device-side wait hang instead of fail:
	// drop them all, the host message that follows the peer's synchronous Trace is ordering enough.
	if (p->ev[0]) {
		bool visible = true;
		for (uint32_t i = 0; i < x->depth && visible; i++) visible = hipEventQuery(p->ev[i]) == hipSuccess;
		if (!visible) {
			(void)hipGetLastError();
			p->drop_events();
			(void)hipGetLastError();
			if (getenv("POLARIS_DEBUG")) fprintf(stderr, "[polaris] ipc_open: the peer's inter-process events do not read complete here; merging on the host-side ordering alone\n");
		}
	}
	p->info.has_events = p->ev[0] ? 1u : 0u;
	*out = p.release();
	return POLARIS_OK;
}

int polaris_hip_peer_info(polaris_hip_peer *p, PolarisPeerInfo *out) {
	if (!p || !out) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "peer_info: null argument");
	if (out->struct_size != sizeof(PolarisPeerInfo)) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "peer_info: struct_size %u, this library's PolarisPeerInfo has %zu bytes", out->struct_size, sizeof(PolarisPeerInfo));
	std::lock_guard<std::mutex> lk(p->owner->fa.mu); // (a merge that finds the peer's events unusable drops them: has_events follows)
	*out = p->info;
	out->has_events = p->ev[0] ? 1u : 0u;
	return POLARIS_OK;
}

int polaris_hip_merge_counts(polaris_hip_tracer *dst, uint64_t counts[POLARIS_MERGE_BRANCHES]) {
	if (!dst || !counts) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge_counts: null argument");
	std::lock_guard<std::mutex> lk(dst->fa.mu);
	for (int i = 0; i < POLARIS_MERGE_BRANCHES; i++) counts[i] = dst->fa.counts[i];
	return POLARIS_OK;
}

int polaris_hip_ipc_close(polaris_hip_tracer *dst, polaris_hip_peer *p) {
	if (!dst || !p) return fail(dst, POLARIS_E_BAD_ARGUMENT, "ipc_close: null argument");
	if (p->owner != dst) return fail(dst, POLARIS_E_BAD_ARGUMENT, "ipc_close: the peer was opened by another tracer");
	std::lock_guard<std::mutex> lk(dst->fa.mu);
	(void)hipSetDevice(dst->device);
	(void)hipStreamSynchronize(dst->fa.q); // a merge may still be reading the mapping
	delete p;
	(void)hipGetLastError();
	return POLARIS_OK;
}

int polaris_hip_export_block(polaris_hip_tracer *h, const PolarisBlockRequest *r, void *device_dst) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (int rc = check_request(h, r)) return rc;
	if (!device_dst) return fail(h, POLARIS_E_BAD_ARGUMENT, "export: destination is null");
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t off = (size_t)r->block_y * h->fa.W, n = (size_t)r->block_h * h->fa.W;
	HIP_TRY(h, hipMemcpyAsync(device_dst, h->fa.current() + off, n * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return POLARIS_OK;
}

int polaris_hip_merge_device(polaris_hip_tracer *dst, const void *device_rows, const PolarisBlockRequest *r) {
	if (!dst) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(dst->mu);
	if (int rc = check_request(dst, r)) return rc;
	if (!device_rows) return fail(dst, POLARIS_E_BAD_ARGUMENT, "merge_device: source is null");
	HIP_TRY(dst, hipSetDevice(dst->device));
	const size_t off = (size_t)r->block_y * dst->fa.W, n = (size_t)r->block_h * dst->fa.W;
	std::lock_guard<std::mutex> lk_merge(dst->fa.mu); // the frame accumulator is the merge stream's
	HIP_TRY(dst, dst->fa.add_rows((const float4 *)device_rows, off, n, dst->opt_moments, route_merge(MergeKind::DeviceStrip, -1, false, -1, false).branch));
	HIP_TRY(dst, hipStreamSynchronize(dst->fa.q)); // the caller owns device_rows: do not outlive it
	return POLARIS_OK;
}

int polaris_hip_reset_frame(polaris_hip_tracer *h) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (h->fa.W == 0 || h->fa.H == 0) return fail(h, POLARIS_E_BAD_ARGUMENT, "frame dimensions not set (UpdateState FrameDimensions)");
	HIP_TRY(h, hipSetDevice(h->device));
	HIP_TRY(h, h->fa.reset_frame());
	return POLARIS_OK;
}

int polaris_hip_reset_epoch(polaris_hip_tracer *h, uint64_t *epoch) {
	if (!h || !epoch) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "reset_epoch: null argument");
	std::lock_guard<std::mutex> lk(h->fa.mu);
	*epoch = h->fa.reset_epoch;
	return POLARIS_OK;
}

int polaris_hip_wait_reset(polaris_hip_tracer *h, uint64_t epoch) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::unique_lock<std::mutex> lk(h->fa.mu);
	// (bounded: a caller that waits for a Trace nobody will issue gets an error instead of a hung thread)
	if (!h->fa.reset_cv.wait_for(lk, std::chrono::seconds(120), [&] { return h->fa.reset_epoch > epoch; })) {
		return h->fa.fail(POLARIS_E_TIMEOUT, "wait_reset: no Trace with accumulated_samples == 0 (or reset_frame) arrived within 120 s");
	}
	return POLARIS_OK;
}

} // extern "C"

namespace {
// The PRIOR plane of a W x H frame on stream q (caller holds mu): the history (hist, hguide, halbedo under hcam; hist = null: none)
// reprojected onto the G-buffer (guide, albedo) under cam.  polaris_hip_sync_framebuffer and polaris_hip_reproject_planes both
// launch it through here.
// prior2 != null (variance guidance on): PRIOR2 too, from the history's VARIANCE plane hvar (null: the history has no M2, PRIOR2 = 0).
// mo != null (object motion): the two INSTANCE planes and the motion table of the instances between the history and now.
// mo->hit != null (vertex motion, the history has a snapshot): the HIT plane, the scene's vertices, the history's and the deformation table.
struct MotionArgs {
	const uint32_t *inst, *hinst; const float4 *table; uint32_t n_inst;
	const uint4 *hit = nullptr; const float4 *verts = nullptr, *hverts = nullptr, *deform = nullptr; uint32_t n_tris = 0;
};
hipError_t launch_reproject(polaris_hip_tracer *h, hipStream_t q, const float4 *hist, const float4 *hguide, const float4 *halbedo, const TpCamera &hcam,
                      const float4 *guide, const float4 *albedo, const TpCamera &cam, uint32_t W, uint32_t H, const PolarisTemporalParams &p,
                      float4 *prior, const float4 *hvar = nullptr, float4 *prior2 = nullptr, const MotionArgs *mo = nullptr, const TpProjection *proj = nullptr) {
	// proj != null (polaris_hip_set_projection is on): both cameras are this projection's, only their eyes are read, and the *_proj kernels run
	const size_t F = (size_t)W * H;
	const bool none = !hist || (!proj && !tp_projectable(hcam)) || p.max_history == 0; // no history anywhere: m = 0
	const bool m2 = prior2 && hvar && !none;                                // (else the PRIOR as without variance guidance, PRIOR2 = 0)
	const bool deform = mo && mo->hit;
	const auto &variant = kReproject[m2][mo != nullptr];
	const char *const symbol = proj ? (deform ? kReprojectDeformProj[m2].symbol : kReprojectProj[m2][mo != nullptr].symbol) : (deform ? kReprojectDeform[m2].symbol : variant.symbol);
	Timed t(h, "reproject", none ? nullptr : symbol, q);
	if (prior2 && !m2)
		if (hipError_t e = hipMemsetAsync(prior2, 0, F * sizeof(float4), q)) return e;
	if (none) return hipMemsetAsync(prior, 0, F * sizeof(float4), q);
	if (proj) {
		const float3 heye = make_float3(hcam.eye[0], hcam.eye[1], hcam.eye[2]), eye = make_float3(cam.eye[0], cam.eye[1], cam.eye[2]);
		if (deform)
			kReprojectDeformProj[m2].enqueue(grid_for(F), WG, 0, q, hist, hguide, halbedo, *proj, heye, guide, albedo, eye, W, H, p.max_history, p.normal_threshold,
			                                 p.depth_threshold, prior, m2 ? hvar : nullptr, m2 ? prior2 : nullptr, mo->inst, mo->hinst, mo->table, mo->n_inst,
			                                 mo->hit, mo->verts, mo->hverts, mo->deform, mo->n_tris);
		else kReprojectProj[m2][mo != nullptr].enqueue(grid_for(F), WG, 0, q, hist, hguide, halbedo, *proj, heye, guide, albedo, eye, W, H, p.max_history,
		                                              p.normal_threshold, p.depth_threshold, prior, m2 ? hvar : nullptr, m2 ? prior2 : nullptr, mo ? mo->inst : nullptr,
		                                              mo ? mo->hinst : nullptr, mo ? mo->table : nullptr, mo ? mo->n_inst : 0u);
		return hipGetLastError();
	}
	if (deform)
		kReprojectDeform[m2].enqueue(grid_for(F), WG, 0, q, hist, hguide, halbedo, hcam, guide, albedo, cam, W, H, p.max_history, p.normal_threshold,
		                             p.depth_threshold, prior, m2 ? hvar : nullptr, m2 ? prior2 : nullptr, mo->inst, mo->hinst, mo->table, mo->n_inst,
		                             mo->hit, mo->verts, mo->hverts, mo->deform, mo->n_tris);
	else variant.enqueue(grid_for(F), WG, 0, q, hist, hguide, halbedo, hcam, guide, albedo, cam, W, H, p.max_history, p.normal_threshold, p.depth_threshold,
	                prior, m2 ? hvar : nullptr, m2 ? prior2 : nullptr, mo ? mo->inst : nullptr, mo ? mo->hinst : nullptr, mo ? mo->table : nullptr,
	                mo ? mo->n_inst : 0u);
	return hipGetLastError();
}

struct SyncIo { // what the steps of a sync read and write: the rows [y0, y1) of planes W wide (tp, prior, prior2: TEMPORAL, PRIOR, PRIOR2 with temporal reuse)
	const float4 *acc; float nf, weight;
	float4 *tp; const float4 *prior, *prior2, *guide, *albedo;
	float4 *var, *ping, *pong, *out; uchar4 *fb;
	uint32_t W, y0, y1; float exposure;
	const DisplayStage *dp = nullptr; // with the display stage in the plan
	const BloomStage *bl = nullptr;   // with bloom in the plan
};

// The pyramid launches of a bloomed sync under one bracket (bloom.h): D_1 .. D_L down -- level 1 from the bright pass of src --, then
// U_{L-1} .. U_1 up in place.  fused: k_bloom_tail takes every level from bl_tail_start on, down and up, in one launch.
void launch_bloom(polaris_hip_tracer *h, hipStream_t q, const float4 *src, float w, float exposure, const float *E, const BlLevels &g, const BloomStage &B) {
	const PolarisBloomParams &p = B.p;
	float4 *pyr = B.pyramid.get();
	const BlBright bp{w, exposure, 1.0f, p.threshold, p.knee}; // (E is read on the device)
	const uint32_t tail = B.fused ? bl_tail_start(g) : g.L + 1;
	const int first = p.karis ? 2 : 1;
	auto tiles = [](uint32_t lw, uint32_t lh) { return dim3((lw + kBlTile - 1) / kBlTile, (lh + kBlTile - 1) / kBlTile); };
	Timed t(h, kSyncStepTimer[(int)SyncStep::Bloom], tail == 1 ? kBloomTail[first].symbol : kBloomDown[first].symbol, q);
	for (uint32_t l = 1; l < tail; l++)
		kBloomDown[l == 1 ? first : 0].enqueue(tiles(g.w[l], g.h[l]), WG, 0, q, l == 1 ? src : pyr + g.off[l - 1], (int)g.w[l - 1], (int)g.h[l - 1], pyr + g.off[l],
		                                       (int)g.w[l], (int)g.h[l], bp, E);
	if (tail <= g.L) kBloomTail[tail == 1 ? first : 0].enqueue(1u, WG, 0, q, src, pyr, g, tail, bp, E);
	for (uint32_t l = std::min(tail, g.L) - 1; l >= 1; l--) // (with a tail: U_tail is in the pyramid)
		kBloomUp.enqueue(tiles(g.w[l], g.h[l]), WG, 0, q, pyr + g.off[l], (int)g.w[l], (int)g.h[l], pyr + g.off[l + 1], (int)g.w[l + 1], (int)g.h[l + 1]);
}

// One of plan_tail's steps (frame_sync.h) on stream q over n pixels of src (rows W wide), read with weight w, into fb: the tone-map, or
// the display stage's k_meter (behind the clear of its histogram), k_expose, the bloom pyramid (B: bloom is in the plan) and k_display
// or k_display_bloom.
constexpr uint32_t kMeterMaxGrid = 128; // k_meter's workgroups stride over the pixels, kMeterUnroll at a time: one flush of a histogram per workgroup
void launch_tail_step(polaris_hip_tracer *h, hipStream_t q, SyncStep step, const float4 *src, float w, uchar4 *fb, size_t n, uint32_t W, float exposure,
                      const DisplayStage *D, const BloomStage *B) {
	const PolarisDisplayParams *p = D ? &D->p : nullptr; // (null: the plan has no display step)
	DpDevice *d = D ? D->dev.get() : nullptr;
	const char *timer = kSyncStepTimer[(int)step];
	if (B && (step == SyncStep::Bloom || step == SyncStep::Display)) { // (B: the plan has the bloom step, so D is there)
		const BlLevels g = bl_levels(W, (uint32_t)(n / W), B->p.levels);
		const float *E = p->auto_exposure ? &d->s.E : &d->one;
		if (step == SyncStep::Bloom) launch_bloom(h, q, src, w, exposure, E, g, *B);
		else (void)launch(h, timer, q, kDisplayBloom[p->tone_operator][p->srgb], grid_for(n), WG, 0, src, fb, (uint32_t)n, W, w, exposure, E, dp_curve(p->white),
		                  (const float4 *)B->pyramid.get() + g.off[1], (int)g.w[1], (int)g.h[1], g.L, B->p.intensity);
		return;
	}
	if (step == SyncStep::Tonemap) (void)launch(h, timer, q, kTonemap, grid_for(n), WG, 0, src, fb, (uint32_t)n, w, exposure);
	else if (step == SyncStep::Meter) {
		Timed t(h, timer, kMeter.symbol, q);
		(void)hipMemsetAsync(d->hist, 0, sizeof d->hist, q);
		kMeter.enqueue(std::min(grid_for((n + kMeterUnroll - 1) / kMeterUnroll), kMeterMaxGrid), WG, 0, q, src, (uint32_t)n, w, d);
	} else if (step == SyncStep::Expose) (void)launch(h, timer, q, kExpose, 1u, 64, 0, d, D->meter());
	else (void)launch(h, timer, q, kDisplay[p->tone_operator][p->srgb], grid_for(n), WG, 0, src, fb, (uint32_t)n, w, exposure,
	                  p->auto_exposure ? &d->s.E : &d->one, dp_curve(p->white));
}

// The timed steps of a sync on stream q, in the plan's order (frame_sync.h plan_sync; caller holds mu): k_temporal into TEMPORAL, k_variance
// into VARIANCE, the filter (variance-guided or not) over the plan's colour -- TEMPORAL with weight 1, or the accumulator with the sync's
// weight -- into DENOISED, and the tone-map of the plan's source.  polaris_hip_sync_framebuffer and the test entries
// polaris_hip_denoise_planes / _variance_planes all launch through here.
void launch_steps(polaris_hip_tracer *h, hipStream_t q, const SyncPlan &P, const SyncIo &io, const PolarisDenoiseParams &p, const PolarisVarianceParams &v) {
	const size_t off = (size_t)io.y0 * io.W, n = (size_t)(io.y1 - io.y0) * io.W;
	const uint32_t grid = grid_for(n), W = io.W, y0 = io.y0, y1 = io.y1;
	const bool temporal = P.color == SyncSource::Temporal, filtered = P.tonemap == SyncSource::Denoised;
	const float4 *c = temporal ? io.tp : io.acc, *tp = temporal ? io.tp : nullptr, *prior2 = temporal ? io.prior2 : nullptr;
	const float cw = temporal ? 1.0f : io.weight;
	// THE a-trous loop: the iterations of one filter variant under one timer bracket, through ping / pong into out.  enqueue(in, dst, it,
	// last) launches iteration `it` from `in` (null: the filter's own input) into dst.
	auto atrous = [&](const char *timer, const char *symbol, float sigma_luminance, auto enqueue) {
		Timed t(h, timer, symbol, q);
		const float4 *in = nullptr;
		for (uint32_t k = 0; k < p.iterations; k++) {
			float4 *dst = k + 1 == p.iterations ? io.out : (k % 2 == 0 ? io.ping : io.pong);
			enqueue(in, dst, dn_iter(k, p.normal_power_log2, p.sigma_depth, sigma_luminance), k + 1 == p.iterations ? 1 : 0);
			in = dst;
		}
	};
	for (int s = 0; s < P.n_steps; s++) {
		const SyncStep step = P.steps[s];
		const char *timer = kSyncStepTimer[(int)step];
		if (step == SyncStep::Temporal) (void)launch(h, timer, q, kTemporal, grid, WG, 0, io.acc, io.prior, io.tp, W, y0, y1, io.nf, io.weight);
		else if (step == SyncStep::Variance)
			(void)launch(h, timer, q, kVariance, grid, WG, 0, io.acc, io.nf, io.weight, tp, prior2, io.guide, io.albedo, io.var, W, y0, y1, dn_iter(0, p.normal_power_log2, p.sigma_depth, 0.0f), v.min_samples);
		else if (step == SyncStep::Denoise)
			atrous(timer, kDenoise.symbol, p.sigma_luminance, [&](const float4 *in, float4 *dst, const DnIter &it, int last) { kDenoise.enqueue(grid, WG, 0, q, c, cw, io.guide, io.albedo, in, dst, W, y0, y1, it, last); });
		else if (step == SyncStep::DenoiseVariance)
			atrous(timer, kDenoiseVariance.symbol, 0.0f, [&](const float4 *in, float4 *dst, const DnIter &it, int last) { kDenoiseVariance.enqueue(grid, WG, 0, q, c, cw, io.var, io.guide, io.albedo, in, dst, W, y0, y1, it, v.sigma_variance, last); });
		else launch_tail_step(h, q, step, (filtered ? io.out : c) + off, filtered ? 1.0f : cw, io.fb + off, n, W, io.exposure, io.dp, io.bl);
	}
}

// What a displayed sync needs on the device (caller holds mu; the main stream is idle): allocated at the first one, and after a reset
// the bins' values, the 1.0f and an empty exposure state uploaded on the main stream.
int ensure_display(polaris_hip_tracer *h) {
	DisplayStage &D = h->fs.dp;
	if (!D.dev) { HIP_TRY(h, D.dev.alloc(1)); D.fresh = false; }
	if (D.fresh) return POLARIS_OK;
	dp_init(D.init, nullptr);
	HIP_TRY(h, hipMemcpyAsync(D.dev, &D.init, sizeof(DpDevice), hipMemcpyHostToDevice, h->stream));
	D.fresh = true;
	return POLARIS_OK;
}

// The pyramid of a bloomed sync (caller holds mu): allocated at the first one for the whole frame, which no request's rows exceed.
int ensure_bloom(polaris_hip_tracer *h) {
	BloomStage &B = h->fs.bl;
	if (B.pyramid) return POLARIS_OK;
	const BlLevels g = bl_levels(h->fa.W, h->fa.H, B.p.levels);
	HIP_TRY(h, B.pyramid.alloc(g.off[g.L + 1]));
	return POLARIS_OK;
}

// What polaris_hip_sync_framebuffer queues with denoising, temporal reuse or variance guidance on (caller holds mu; request checked), by
// the plan of frame_sync.h: G-buffer if stale, the planes the features need, TEMPORAL / VARIANCE cleared at their first sync under this
// camera, PRIOR if stale, the merges queued so far, then the timed steps over the request's rows.
int enqueue_features(polaris_hip_tracer *h, const PolarisBlockRequest *r, float weight, const SyncFeatures &f) {
	FrameSync &S = h->fs;
	if (!h->camera.have_camera)
		return fail(h, POLARIS_E_BAD_ARGUMENT, "%s needs the camera (UpdateState CameraData)", f.temporal ? "temporal reuse" : (f.variance ? "variance guidance" : "denoising"));
	const SyncPlan P = plan_sync(f, S.v);
	if (int rc = ensure_gbuffer(h)) return rc;
	if (int rc = ensure_planes(h, P.need, P.clear, P.clear_new)) return rc;
	if (P.prior) {
		MotionArgs mo{};
		if (P.motion && (S.v.hist.inv.size() != S.v.cur.inv.size() || S.v.cur.mesh_index.empty() || !S.tp_hinst || !S.gb_inst))
			return fail(h, POLARIS_E_DEVICE, "temporal sync: the history's instance table does not fit the scene's"); // (cannot happen: upload_scene drops such a history)
		if (P.motion) {
			const uint32_t n_inst = (uint32_t)S.v.cur.mesh_index.size();
			S.mo_table_host.resize((size_t)n_inst * 16);
			tp_motion_table(n_inst, S.v.hist.inv.data(), S.v.cur.inv.data(), S.mo_table_host.data());
			HIP_TRY(h, S.mo_table.reserve((size_t)n_inst * 4)); // (the main stream is idle: every sync ends with its synchronisation)
			HIP_TRY(h, hipMemcpyAsync(S.mo_table, S.mo_table_host.data(), S.mo_table_host.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
			mo = MotionArgs{S.gb_inst, S.tp_hinst, S.mo_table, n_inst};
			if (P.deform) { // the history has a snapshot of the vertices: its instances' mesh -> world beside the motion table
				if (!S.gb_hit || !S.vert_snap || !h->ds.vup.on || S.vert_snap.capacity() < (size_t)h->ds.vup.num_triangles * 3)
					return fail(h, POLARIS_E_DEVICE, "temporal sync: the history's vertices do not fit the scene's"); // (cannot happen: the topology is the history's)
				S.de_table_host.resize((size_t)n_inst * 16);
				tp_deform_table(n_inst, S.v.hist.inv.data(), S.de_table_host.data());
				HIP_TRY(h, S.de_table.reserve((size_t)n_inst * 4));
				HIP_TRY(h, hipMemcpyAsync(S.de_table, S.de_table_host.data(), S.de_table_host.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
				mo.hit = S.gb_hit; mo.verts = h->ds.vup.vertices; mo.hverts = S.vert_snap; mo.deform = S.de_table; mo.n_tris = h->ds.vup.num_triangles;
			}
		}
		const TpProjection proj = projection_args(h->camera); // (read only while the projection is on)
		HIP_TRY(h, launch_reproject(h, h->stream, P.history ? S.pl[kTpHist].get() : nullptr, S.pl[kTpHGuide], S.pl[kTpHAlbedo], tp_camera(S.tp_hcam.eye, S.tp_hcam.frustum),
		                            S.pl[kGuide], S.pl[kAlbedo], tp_camera(h->camera.open.eye, h->camera.open.frustum), h->fa.W, h->fa.H, S.tp, S.pl[kTpPrior],
		                            P.m2 ? S.pl[kVaHist].get() : nullptr, f.variance ? S.pl[kTpPrior2].get() : nullptr, P.motion ? &mo : nullptr,
		                            h->camera.projection_on() ? &proj : nullptr));
		S.v.prior_computed();
	}
	HIP_TRY(h, h->fa.join_merges(h->stream)); // (as the plain sync: the merges queued so far are part of the frame)
	launch_steps(h, h->stream, P, SyncIo{h->fa.frame, (float)(r->accumulated_samples + r->samples_per_pixel), weight, S.pl[kTpOut], S.pl[kTpPrior], S.pl[kTpPrior2],
	                                     S.pl[kGuide], S.pl[kAlbedo], S.pl[kVaOut], S.pl[kDnPing], S.pl[kDnPong], S.pl[kDnOut], h->framebuffer, h->fa.W, r->block_y,
	                                     r->block_y + r->block_h, r->exposure, f.display ? &S.dp : nullptr, f.bloomed() ? &S.bl : nullptr}, S.dn, S.va);
	return POLARIS_OK;
}

// The scratch of a *_planes test entry, which reads and writes no tracer state: one allocation carved into n4 float4 planes of F pixels
// followed by n1 planes of F words (an INSTANCE plane, or RGBA8 pixels), and lists of copies on the main stream, which is drained
// before the memory goes on every way out.
struct PlaneScratch {
	struct Copy { void *dst; const void *src; size_t bytes; }; // (either null: skipped)
	hipStream_t q; size_t F, n4 = 0;
	DevArray<char> mem;
	StreamDrain drain{q}; // (declared after the memory)
	hipError_t alloc(size_t n4_, size_t n1) { n4 = n4_; return mem.alloc((n4 * sizeof(float4) + n1 * sizeof(uint32_t)) * F); }
	float4 *f4(size_t i) const { return (float4 *)mem.get() + i * F; }
	uint32_t *word(size_t i) const { return (uint32_t *)f4(n4) + i * F; }
	hipError_t copy(hipMemcpyKind kind, std::initializer_list<Copy> list) const {
		for (const Copy &c : list)
			if (c.dst && c.src)
				if (hipError_t e = hipMemcpyAsync(c.dst, c.src, c.bytes, kind, q)) return e;
		return hipSuccess;
	}
};

// The refusal of a *_planes test entry (caller holds mu): the entry, the text of the broken rule (reproject_io.h, or the entry's own
// about its params) and the numbers the rules are about.
int refuse_planes(polaris_hip_tracer *h, const char *name, const char *rule, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h) {
	return fail(h, POLARIS_E_BAD_ARGUMENT, "%s: %s (frame %ux%u, rows [%u, +%u))", name, rule, W, H, block_y, block_h);
}
const char *frame_rows_rule(uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h) { // (null: both hold)
	int rule = check_frame(W, H);
	if (!rule) rule = check_rows(H, block_y, block_h);
	return rule ? plane_rule_text(rule) : nullptr;
}

PolarisExposureInfo exposure_info(const DpDevice &d) {
	return PolarisExposureInfo{sizeof(PolarisExposureInfo), d.s.valid, (uint64_t)d.s.n_hi << 32 | d.s.n_lo, d.s.avg, d.s.log2E, d.s.E, 0};
}

// THE body of polaris_hip_denoise_planes (variance = null: no VARIANCE plane) and polaris_hip_variance_planes (arguments checked; caller holds
// mu): the planes of a sync with the features f uploaded, its steps over the rows, VARIANCE (if any), DENOISED and the frame read back.
int filter_planes_entry(polaris_hip_tracer *h, const SyncFeatures &f, const float *acc, const float *guide, const float *albedo, uint32_t W, uint32_t H,
                        uint32_t block_y, uint32_t block_h, float nf, float weight, float exposure, const PolarisDenoiseParams &p,
                        const PolarisVarianceParams &v, float *variance, float *denoised, uint8_t *rgba) {
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t F = (size_t)W * H, plane = F * sizeof(float4), pixels = F * sizeof(uchar4);
	PlaneScratch d{h->stream, F};
	HIP_TRY(h, d.alloc(variance ? 7 : 6, 1));
	float4 *d_acc = d.f4(0), *d_guide = d.f4(1), *d_albedo = d.f4(2), *d_ping = d.f4(3), *d_pong = d.f4(4), *d_out = d.f4(5), *d_var = variance ? d.f4(6) : nullptr;
	uchar4 *d_fb = (uchar4 *)d.word(0);
	HIP_TRY(h, d.copy(hipMemcpyHostToDevice, {{d_acc, acc, plane}, {d_guide, guide, plane}, {d_albedo, albedo, plane}, {d_var, variance, plane}, {d_out, denoised, plane},
	                                          {d_fb, rgba, pixels}}));
	launch_steps(h, h->stream, plan_sync(f, SyncState()),
	             SyncIo{d_acc, nf, weight, nullptr, nullptr, nullptr, d_guide, d_albedo, d_var, d_ping, d_pong, d_out, d_fb, W, block_y, block_y + block_h, exposure}, p, v);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, d.copy(hipMemcpyDeviceToHost, {{variance, d_var, plane}, {denoised, d_out, plane}, {rgba, d_fb, pixels}}));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	collect_timers(h);
	return POLARIS_OK;
}

// THE body of polaris_hip_display_planes (bp = null: display only) and polaris_hip_bloom_planes: the tail of a displayed sync over the
// rows of a caller plane, on a display stage (and a pyramid) of its own.
int display_planes_entry(polaris_hip_tracer *h, const char *name, const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight,
                         float exposure, const PolarisDisplayParams *dp, const PolarisBloomParams *bp, bool bloom, const float *prev_log2E, uint8_t *rgba,
                         uint32_t histogram[256], PolarisExposureInfo *info, float *level1, uint32_t *levels_used) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const char *rule = !plane || !rgba || !dp || (bloom && !bp) ? plane_rule_text(kRuleNull) : frame_rows_rule(W, H, block_y, block_h);
	if (!rule && (dp->struct_size != sizeof(PolarisDisplayParams) || !dp->enabled || dp_check(*dp)))
		rule = "params polaris_hip_set_display refuses (enabled must be 1)";
	if (!rule && bloom && (bp->struct_size != sizeof(PolarisBloomParams) || !bp->enabled || bl_check(*bp)))
		rule = "params polaris_hip_set_bloom refuses (enabled must be 1)";
	if (!rule && info && info->struct_size != sizeof(PolarisExposureInfo)) rule = "info's struct_size";
	if (rule) return refuse_planes(h, name, rule, W, H, block_y, block_h);
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t F = (size_t)W * H, off = (size_t)block_y * W, n = (size_t)block_h * W;
	const BlLevels g = bloom ? bl_levels(W, block_h, bp->levels) : BlLevels{};
	const bool metered = histogram || info;
	DisplayStage D; // (its device state and the pyramid go after the stream is drained)
	BloomStage B;
	DpDevice got;   // D.init and got are the source and target of asynchronous copies: all are declared before d, whose StreamDrain waits
	                // for the stream on every way out, early returns included, before any of them leaves scope
	PlaneScratch d{h->stream, F};
	HIP_TRY(h, d.alloc(1, 1));
	HIP_TRY(h, D.dev.alloc(1));
	if (bloom) HIP_TRY(h, B.pyramid.alloc(g.off[g.L + 1]));
	D.p = *dp;
	if (bloom) B.p = *bp;
	B.fused = h->fs.bl.fused;
	dp_init(D.init, prev_log2E);
	float4 *d_plane = d.f4(0);
	uchar4 *d_fb = (uchar4 *)d.word(0);
	HIP_TRY(h, d.copy(hipMemcpyHostToDevice, {{d_plane, plane, F * sizeof(float4)}, {d_fb, rgba, F * sizeof(uchar4)}, {D.dev.get(), &D.init, sizeof(DpDevice)}}));
	SyncFeatures f;
	f.display = true;
	f.bloom = bloom;
	f.auto_exposure = dp->auto_exposure != 0;
	SyncStep steps[kMaxSyncSteps];
	const int n_steps = plan_tail(f, steps, 0);
	for (int s = 0; s < n_steps; s++) launch_tail_step(h, h->stream, steps[s], d_plane + off, weight, d_fb + off, n, W, exposure, &D, bloom ? &B : nullptr);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, d.copy(hipMemcpyDeviceToHost, {{rgba, d_fb, F * sizeof(uchar4)}, {metered ? &got : nullptr, D.dev.get(), sizeof got},
	                                          {level1, bloom ? B.pyramid.get() + g.off[1] : nullptr, (size_t)g.w[1] * g.h[1] * sizeof(float4)}}));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	collect_timers(h);
	if (histogram) memcpy(histogram, got.hist, sizeof got.hist);
	if (info) *info = exposure_info(got);
	if (levels_used) *levels_used = g.L;
	return POLARIS_OK;
}

// THE body of polaris_hip_reproject_planes, _reproject_motion_planes and _reproject_deform_planes: the PRIOR (and PRIOR2) of a
// description, by the kernel launch_reproject selects for its groups.  Reads and writes no tracer state.
int reproject_planes_entry(polaris_hip_tracer *h, const char *name, const ReprojectIo &io) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (const int rule = check_reproject(io))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "%s: %s (frame %ux%u, %u instances, %u triangles)", name, plane_rule_text(rule), io.W, io.H, io.n_instances, io.num_triangles);
	HIP_TRY(h, hipSetDevice(h->device));
	const bool motion = io.motion(), deform = io.deform();
	const uint32_t ni = io.n_instances;
	const size_t F = (size_t)io.W * io.H, plane = F * sizeof(float4), words = F * sizeof(uint32_t), nv = (size_t)io.num_triangles * 3;
	std::vector<float> table((size_t)ni * (deform ? 32 : 16)); // the motion table, then the deformation table
	if (motion) tp_motion_table(ni, io.prev_inv_transforms, io.inv_transforms, table.data());
	if (deform) tp_deform_table(ni, io.prev_inv_transforms, table.data() + (size_t)ni * 16);
	DevArray<float4> d_table, d_verts;
	PlaneScratch d{h->stream, F}; // (declared after the tables and the side arrays: its StreamDrain waits for the stream on every way out,
	                              // early returns included, before the memory and the host vector that asynchronous copies read leave scope)
	HIP_TRY(h, d.alloc(deform ? 9 : (motion ? 8 : 6), motion ? 2 : 0)); // (the ninth float4 plane holds the HIT words)
	if (motion) HIP_TRY(h, d_table.alloc((size_t)ni * (deform ? 8 : 4)));
	if (deform) HIP_TRY(h, d_verts.alloc(2 * nv));
	float4 *d_hist = d.f4(0), *d_hguide = d.f4(1), *d_halbedo = d.f4(2), *d_guide = d.f4(3), *d_albedo = d.f4(4), *d_prior = d.f4(5);
	float4 *d_hvar = io.m2() ? d.f4(6) : nullptr, *d_prior2 = io.m2() ? d.f4(7) : nullptr;
	uint4 *d_hit = deform ? (uint4 *)d.f4(8) : nullptr;
	uint32_t *d_hinst = motion ? d.word(0) : nullptr, *d_inst = motion ? d.word(1) : nullptr;
	HIP_TRY(h, d.copy(hipMemcpyHostToDevice, {{d_hist, io.history, plane}, {d_hguide, io.prev_guide, plane}, {d_halbedo, io.prev_albedo, plane}, {d_guide, io.guide, plane},
	                                          {d_albedo, io.albedo, plane}, {d_hvar, io.history_variance, plane}, {d_hinst, io.prev_instance, words}, {d_inst, io.instance, words},
	                                          {d_hit, io.hit, F * sizeof(uint4)}, {d_table.get(), table.data(), table.size() * sizeof(float)},
	                                          {d_verts.get(), io.vertices, nv * sizeof(float4)}, {deform ? d_verts.get() + nv : nullptr, io.prev_vertices, nv * sizeof(float4)}}));
	MotionArgs mo{d_inst, d_hinst, d_table, ni};
	if (deform) { mo.hit = d_hit; mo.verts = d_verts; mo.hverts = d_verts.get() + nv; mo.deform = d_table.get() + (size_t)ni * 4; mo.n_tris = io.num_triangles; }
	HIP_TRY(h, launch_reproject(h, h->stream, d_hist, d_hguide, d_halbedo, tp_camera(io.prev_eye, io.prev_frustum), d_guide, d_albedo, tp_camera(io.eye, io.frustum),
	                            io.W, io.H, *io.p, d_prior, d_hvar, d_prior2, motion ? &mo : nullptr));
	HIP_TRY(h, d.copy(hipMemcpyDeviceToHost, {{io.prior, d_prior, plane}, {io.prior2, d_prior2, plane}}));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	collect_timers(h);
	return POLARIS_OK;
}
} // namespace

extern "C" {

int polaris_hip_set_denoise(polaris_hip_tracer *h, const PolarisDenoiseParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!p || p->struct_size != sizeof(PolarisDenoiseParams))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_denoise: null params or struct_size != %zu", sizeof(PolarisDenoiseParams));
	if (dn_check(p->iterations, p->normal_power_log2, p->sigma_depth, p->sigma_luminance))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_denoise: iterations %u (0..%u), normal_power_log2 %u (0..%u), sigmas %g / %g (0 or [%g, %g])",
		            p->iterations, kDnMaxIterations, p->normal_power_log2, kDnMaxNormalPowerLog2, (double)p->sigma_depth,
		            (double)p->sigma_luminance, (double)kDnSigmaMin, (double)kDnSigmaMax);
	h->fs.dn = *p;
	return POLARIS_OK;
}

int polaris_hip_set_temporal(polaris_hip_tracer *h, const PolarisTemporalParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!p || p->struct_size != sizeof(PolarisTemporalParams))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_temporal: null params or struct_size != %zu", sizeof(PolarisTemporalParams));
	if (tp_check(p->max_history, p->normal_threshold, p->depth_threshold))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_temporal: max_history %u (0..%u), normal_threshold %g ([-1, 1]), depth_threshold %g ([0, %g])",
		            p->max_history, kTpMaxHistory, (double)p->normal_threshold, (double)p->depth_threshold, (double)kTpMaxDepthThreshold);
	if (p->max_history == 0 && h->fs.tp.max_history) { // its planes go
		HIP_TRY(h, hipSetDevice(h->device));
		HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every temporal launch is on the main stream)
	}
	h->fs.set_temporal(*p);
	return POLARIS_OK;
}

int polaris_hip_set_variance(polaris_hip_tracer *h, const PolarisVarianceParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!p || p->struct_size != sizeof(PolarisVarianceParams))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_variance: null params or struct_size != %zu", sizeof(PolarisVarianceParams));
	if (va_check(p->sigma_variance, p->min_samples))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_variance: sigma_variance %g (0 or [%g, %g]), min_samples %u (1..%u)", (double)p->sigma_variance,
		            (double)kDnSigmaMin, (double)kDnSigmaMax, p->min_samples, kVaMaxMinSamples);
	const bool on = p->sigma_variance != 0.0f, was = h->fs.va.sigma_variance != 0.0f;
	if (on && !h->opt_moments) return fail(h, POLARIS_E_BAD_ARGUMENT, "set_variance: variance guidance needs the option moments = 1 first");
	if (!on && was) { // its planes go
		HIP_TRY(h, hipSetDevice(h->device));
		HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every variance launch is on the main stream)
	}
	h->fs.set_variance(*p);
	return POLARIS_OK;
}

int polaris_hip_set_display(polaris_hip_tracer *h, const PolarisDisplayParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!p || p->struct_size != sizeof(PolarisDisplayParams))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_display: null params or struct_size != %zu", sizeof(PolarisDisplayParams));
	if (dp_check(*p))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_display: enabled %u, srgb %u, auto_exposure %u (0 or 1), tone_operator %u (0..3), white %g ([%g, %g]), key %g "
		            "([%g, %g]), compensation_ev %g, min_ev %g <= max_ev %g ([%g, %g]), permille %u < %u (<= 1000), adapt %g ((0, 1])", p->enabled, p->srgb,
		            p->auto_exposure, p->tone_operator, (double)p->white, (double)kDpMinWhite, (double)kDpMaxWhite, (double)p->key, (double)kDpMinKey,
		            (double)kDpMaxKey, (double)p->compensation_ev, (double)p->min_ev, (double)p->max_ev, -(double)kDpMaxEv, (double)kDpMaxEv, p->low_permille,
		            p->high_permille, (double)p->adapt);
	DisplayStage &D = h->fs.dp;
	if ((!p->enabled && !D.p.enabled) || memcmp(p, &D.p, sizeof *p) == 0) return POLARIS_OK; // (any two off states are equal)
	if (!p->enabled) { // its device state goes, the bloom pyramid with it
		HIP_TRY(h, hipSetDevice(h->device));
		HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every display launch is on the main stream)
		D.dev.reset();
		h->fs.bl.pyramid.reset();
	}
	D.p = *p;
	D.reset();
	return POLARIS_OK;
}

int polaris_hip_set_bloom(polaris_hip_tracer *h, const PolarisBloomParams *p) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!p || p->struct_size != sizeof(PolarisBloomParams))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_bloom: null params or struct_size != %zu", sizeof(PolarisBloomParams));
	if (bl_check(*p))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "set_bloom: enabled %u, karis %u (0 or 1), levels %u (1..%u), threshold %g ([0, %g]), knee %g ([0, 1]), intensity %g ([0, %g])",
		            p->enabled, p->karis, p->levels, kBlMaxLevels, (double)p->threshold, (double)kBlMaxThreshold, (double)p->knee, (double)p->intensity,
		            (double)kBlMaxIntensity);
	BloomStage &B = h->fs.bl;
	if ((!p->enabled && !B.p.enabled) || memcmp(p, &B.p, sizeof *p) == 0) return POLARIS_OK; // (any two off states are equal)
	if (B.pyramid) { // the pyramid goes: off, or its levels may differ
		HIP_TRY(h, hipSetDevice(h->device));
		HIP_TRY(h, hipStreamSynchronize(h->stream)); // (every bloom launch is on the main stream)
		B.pyramid.reset();
	}
	B.p = *p;
	return POLARIS_OK;
}

int polaris_hip_read_exposure(polaris_hip_tracer *h, PolarisExposureInfo *out, uint32_t histogram[256]) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!out || out->struct_size != sizeof(PolarisExposureInfo))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "read_exposure: null info or struct_size != %zu", sizeof(PolarisExposureInfo));
	DisplayStage &D = h->fs.dp;
	if (!D.metered || !D.dev) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_exposure: no sync with auto-exposure on since the exposure state was last reset");
	HIP_TRY(h, hipSetDevice(h->device));
	DpDevice got;
	HIP_TRY(h, hipMemcpyAsync(&got, D.dev, sizeof got, hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	*out = exposure_info(got);
	if (histogram) memcpy(histogram, got.hist, sizeof got.hist);
	return POLARIS_OK;
}

int polaris_hip_read_aov(polaris_hip_tracer *h, int which, float *out, size_t n_floats) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const size_t need = (size_t)h->fa.W * h->fa.H * 4;
	if (!out || n_floats < need || need == 0 || which < POLARIS_AOV_GUIDE || which > POLARIS_AOV_PRIOR2)
		return fail(h, POLARIS_E_BAD_ARGUMENT, "read_aov: need %zu floats, which in {0,1,2,3,4,5,6}", need);
	HIP_TRY(h, hipSetDevice(h->device));
	if (const char *why = h->fs.v.aov_refusal(which, h->fs.tp.max_history != 0, h->fs.pl[kTpPrior2] != nullptr)) return fail(h, POLARIS_E_BAD_ARGUMENT, "%s", why);
	if (which == POLARIS_AOV_GUIDE || which == POLARIS_AOV_ALBEDO) { // computed on demand
		if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
		if (!h->camera.have_camera) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_aov: camera not set");
		if (int rc = ensure_gbuffer(h)) return rc;
	}
	HIP_TRY(h, hipMemcpyAsync(out, h->fs.pl[which], need * sizeof(float), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	collect_timers(h);
	return POLARIS_OK;
}

int polaris_hip_sync_framebuffer(polaris_hip_tracer *h, const PolarisBlockRequest *r) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded"); // tracer.go:254-256
	if (int rc = check_request(h, r)) return rc;
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t off = (size_t)r->block_y * h->fa.W, n = (size_t)r->block_h * h->fa.W;
	const float weight = (float)(1.0 / (float)(r->accumulated_samples + r->samples_per_pixel)); // resources.go:347
	const SyncFeatures f = h->fs.features();
	if (f.display)
		if (int rc = ensure_display(h)) return rc;
	if (f.bloomed())
		if (int rc = ensure_bloom(h)) return rc;
	if (f.any()) {
		if (int rc = enqueue_features(h, r, weight, f)) return rc;
	} else {
		HIP_TRY(h, h->fa.join_merges(h->stream)); // "wait for pending merges" (tracer.go:258-262): everything queued on the merge stream so far
		SyncStep steps[kMaxSyncSteps]; // the tone-map, or the display stage's steps
		const int n_steps = plan_tail(f, steps, 0);
		for (int s = 0; s < n_steps; s++)
			launch_tail_step(h, h->stream, steps[s], h->fa.frame + off, weight, h->framebuffer + off, n, h->fa.W, r->exposure, f.display ? &h->fs.dp : nullptr,
			                 f.bloomed() ? &h->fs.bl : nullptr);
	}
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	if (f.any()) h->fs.v.synced(f);
	if (f.metered()) h->fs.dp.metered = true;
	collect_timers(h);
	return POLARIS_OK;
}

int polaris_hip_read_framebuffer(polaris_hip_tracer *h, uint8_t *rgba, size_t n_bytes) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const size_t need = (size_t)h->fa.W * h->fa.H * 4;
	if (!rgba || n_bytes < need || need == 0) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_framebuffer: need %zu bytes", need);
	HIP_TRY(h, hipSetDevice(h->device));
	HIP_TRY(h, hipMemcpyAsync(rgba, h->framebuffer, need, hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return POLARIS_OK;
}

int polaris_hip_read_accumulator(polaris_hip_tracer *h, int which, float *out, size_t n_floats) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const size_t need = (size_t)h->fa.W * h->fa.H * 4;
	if (!out || n_floats < need || need == 0 || which < 0 || which > 1)
		return fail(h, POLARIS_E_BAD_ARGUMENT, "read_accumulator: need %zu floats, which in {0,1}", need);
	HIP_TRY(h, hipSetDevice(h->device));
	if (which == 1) HIP_TRY(h, h->fa.join_merges(h->stream));
	HIP_TRY(h, hipMemcpyAsync(out, which == 0 ? h->fa.current() : h->fa.frame, need * sizeof(float), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return POLARIS_OK;
}

int polaris_hip_tap_primary(polaris_hip_tracer *h, const PolarisBlockRequest *r, uint32_t seed, float *rays, int32_t *hit,
                            float *wuvt, int32_t *tri) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
	if (int rc = check_request(h, r)) return rc;
	if (!h->camera.have_camera) return fail(h, POLARIS_E_BAD_ARGUMENT, "camera not set");
	const uint32_t N = h->fa.W * r->block_h, Npad = (N + WG - 1) / WG * WG;
	HIP_TRY(h, hipSetDevice(h->device));
	if (int rc = ensure_streams(h, 0, std::max<size_t>(h->pipe[0].slots, Npad), true)) return rc;
	Streams &st0 = h->pipe[0].st;
	st0.hit12 = 0; // (the tap returns the hit distance: 16-byte records)
	st0.o12 = 0;
	if (h->d_seeds.capacity() < 1) HIP_TRY(h, h->d_seeds.alloc(64));
	hipStream_t q = h->stream;
	std::vector<float4> ro(N), rd(N), ht(N);
	std::vector<int> inst(N);
	StreamDrain drain{q}; // (`seed` and the vectors are read and written by asynchronous copies)
	HIP_TRY(h, hipMemcpyAsync(h->d_seeds, &seed, sizeof seed, hipMemcpyHostToDevice, q));
	(void)launch_generate(h, nullptr, q, st0, 1u, 0u, Npad / WG, N, Npad, r->block_y, 1, 1);
	(void)launch_traversal(h, nullptr, tap_traversal(plan_scene(h)), RayKind::Closest, q, st0, 0, Npad / WG, nullptr);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipMemcpyAsync(ro.data(), st0.ray_o, N * sizeof(float4), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipMemcpyAsync(rd.data(), st0.ray_d, N * sizeof(float4), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipMemcpyAsync(ht.data(), st0.hit, N * sizeof(float4), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipMemcpyAsync(inst.data(), st0.hit_inst, N * sizeof(int), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipStreamSynchronize(q));
	for (uint32_t i = 0; i < N; i++) {
		int t;
		memcpy(&t, &ht[i].w, 4);
		if (rays) {
			int pw;
			memcpy(&pw, &rd[i].w, 4);
			float *o = rays + 8 * (size_t)i;
			o[0] = ro[i].x; o[1] = ro[i].y; o[2] = ro[i].z; o[3] = ro[i].w;
			o[4] = rd[i].x; o[5] = rd[i].y; o[6] = rd[i].z; o[7] = (float)(pw & 0xFFFFFF); // util/ray.cl:11
		}
		if (hit) hit[i] = t >= 0 ? 1 : 0;
		if (t >= 0) t &= (int)((1u << h->ds.scene.tri_bits) - 1u); // (the shading class rides above the triangle index)
		if (t >= 0) {
			if (wuvt) {
				float *o = wuvt + 4 * (size_t)i;
				o[0] = 1.0f - (ht[i].x + ht[i].y); o[1] = ht[i].x; o[2] = ht[i].y; o[3] = ht[i].z; // intersect.cl:283-288
			}
			if (tri) { tri[2 * (size_t)i] = inst[i]; tri[2 * (size_t)i + 1] = t; }
		}
	}
	return POLARIS_OK;
}

int polaris_hip_probe(polaris_hip_tracer *h, int kind, uint32_t index, uint32_t n, const float *in, float *out) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
	if (kind < 0 || kind > 3 || (n && (!in || !out))) return fail(h, POLARIS_E_BAD_ARGUMENT, "probe: bad kind or null buffers");
	const uint32_t limit = (kind == kProbeBxdf || kind == kProbeMaterial) ? h->ds.scene.num_nodes : (kind == kProbeTexture ? h->ds.scene.num_textures : h->ds.scene.num_emissives);
	if (index >= limit) return fail(h, POLARIS_E_BAD_ARGUMENT, "probe: index %u out of range (%u)", index, limit);
	if (n == 0) return POLARIS_OK;
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t nin = (size_t)n * kProbeIn[kind], nout = (size_t)n * kProbeOut[kind];
	hipStream_t q = h->stream;
	DevArray<float> d_in, d_out;
	StreamDrain drain{q};
	HIP_TRY(h, d_in.alloc(nin));
	HIP_TRY(h, d_out.alloc(nout));
	HIP_TRY(h, hipMemcpyAsync(d_in, in, nin * sizeof(float), hipMemcpyHostToDevice, q));
	if (tables_staged(h->opt, plan_scene(h))) hipLaunchKernelGGL(k_probe<true>, dim3(grid_for(n)), dim3(WG), 0, q, h->ds.scene, kind, index, n, d_in, d_out);
	else hipLaunchKernelGGL(k_probe<false>, dim3(grid_for(n)), dim3(WG), 0, q, h->ds.scene, kind, index, n, d_in, d_out);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipMemcpyAsync(out, d_out, nout * sizeof(float), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipStreamSynchronize(q));
	return POLARIS_OK;
}

int polaris_hip_probe_intersect(polaris_hip_tracer *h, const float *rays, uint32_t n, int any_hit, int32_t *hit, float *wuvt, int32_t *tri) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
	if (n && (!rays || !hit)) return fail(h, POLARIS_E_BAD_ARGUMENT, "probe_intersect: null buffers");
	if (n > (1u << 24)) return fail(h, POLARIS_E_BAD_ARGUMENT, "probe_intersect: at most 2^24 rays per call");
	if (n == 0) return POLARIS_OK;
	for (uint32_t i = 0; i < n; i++) // (what the tracer's own rays satisfy by construction; the triangle tests rely on it: kernels.h, rcp_det)
		for (int k = 0; k < 3; k++)
			if (!(std::fabs(rays[8 * (size_t)i + k]) <= kMaxCoordinate) || !(std::fabs(rays[8 * (size_t)i + 4 + k]) <= 1024.0f))
				return fail(h, POLARIS_E_BAD_ARGUMENT, "probe_intersect: ray %u: origin beyond 2^40 or direction component beyond 2^10 (or not finite)", i);
	HIP_TRY(h, hipSetDevice(h->device));
	const uint32_t npad = (n + WG - 1) / WG * WG, wgs = npad / WG;
	if (int rc = ensure_streams(h, 0, std::max<size_t>(h->pipe[0].slots, npad), false)) return rc;
	polaris_hip_tracer::Pipe &P = h->pipe[0];
	P.st.hit12 = 0; // (the probe returns the hit distance: 16-byte records)
	P.st.o12 = 0;   // (... and takes arbitrary max distances)
	hipStream_t q = P.q;
	DevArray<float> d_rays;
	std::vector<float4> res(n);
	StreamDrain drain{q};
	HIP_TRY(h, d_rays.alloc((size_t)n * 8));
	HIP_TRY(h, hipMemcpyAsync(d_rays, rays, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice, q));
	hipLaunchKernelGGL(k_probe_rays, dim3(wgs), dim3(WG), 0, q, P.st, d_rays, n, any_hit ? 1 : 0);
	// the traversal kernel the options select for bounce rays (any_hit: shadow rays; trace_plan.h, probe_traversal)
	const RayKind kind = any_hit ? RayKind::AnyHit : RayKind::Closest;
	(void)launch_traversal(h, nullptr, probe_traversal(h->opt, kind), kind, q, P.st, probe_grid(plan_scene(h), any_hit != 0, wgs), wgs, any_hit ? P.st.lsum : nullptr);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipMemcpyAsync(res.data(), any_hit ? P.st.lsum : P.st.hit, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, q));
	HIP_TRY(h, hipStreamSynchronize(q));
	for (uint32_t i = 0; i < n; i++) {
		if (any_hit) { hit[i] = res[i].x == 0.0f ? 1 : 0; continue; } // occluded rays leave their cell untouched
		int t;
		memcpy(&t, &res[i].w, 4);
		hit[i] = t >= 0 ? 1 : 0;
		if (t >= 0) t &= (int)((1u << h->ds.scene.tri_bits) - 1u);
		if (t >= 0 && wuvt) { float *o = wuvt + 4 * (size_t)i; o[0] = 1.0f - (res[i].x + res[i].y); o[1] = res[i].x; o[2] = res[i].y; o[3] = res[i].z; } // intersect.cl:283-288
		if (tri) tri[i] = t;
	}
	return POLARIS_OK;
}

int polaris_hip_selftest_rcp(polaris_hip_tracer *h, float lo, float hi, uint64_t *mismatches_inside, uint64_t *mismatches_outside, uint32_t *sample) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!mismatches_inside || !mismatches_outside) return fail(h, POLARIS_E_BAD_ARGUMENT, "selftest_rcp: null outputs");
	HIP_TRY(h, hipSetDevice(h->device));
	unsigned long long res[3] = {0, 0, 0};
	DevArray<unsigned long long> d;
	StreamDrain drain{h->stream};
	HIP_TRY(h, d.alloc(3));
	HIP_TRY(h, hipMemcpyAsync(d, res, sizeof res, hipMemcpyHostToDevice, h->stream));
	hipLaunchKernelGGL(k_rcp_sweep, dim3((uint32_t)h->num_cus * 32u), dim3(WG), 0, h->stream, lo, hi, d);
	HIP_TRY(h, hipGetLastError());
	HIP_TRY(h, hipMemcpyAsync(res, d, sizeof res, hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	*mismatches_inside = res[0];
	*mismatches_outside = res[1];
	if (sample) *sample = (uint32_t)res[2];
	return POLARIS_OK;
}

int polaris_hip_selftest_builtins(polaris_hip_tracer *h, uint32_t fn, uint64_t first, uint64_t count, uint64_t *fingerprints, uint32_t *results) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const uint64_t chunk = 1ull << PB_CHUNK_LOG2;
	if (fn >= PB_NUM_FN || count == 0 || first > pb_inputs(fn) || count > pb_inputs(fn) - first || (!fingerprints && !results) ||
	    (fingerprints && first % chunk) || (results && count > (1ull << POLARIS_SELFTEST_MAX_RESULTS_LOG2)))
		return fail(h, POLARIS_E_BAD_ARGUMENT, "selftest_builtins: fn %u (< %u), inputs [%llu, +%llu) of %llu, fingerprints from a chunk start, "
		            "at most 2^%d results", fn, (unsigned)PB_NUM_FN, (unsigned long long)first, (unsigned long long)count,
		            (unsigned long long)(fn < PB_NUM_FN ? pb_inputs(fn) : 0), POLARIS_SELFTEST_MAX_RESULTS_LOG2);
	HIP_TRY(h, hipSetDevice(h->device));
	const size_t n_fp = fingerprints ? 2 * (size_t)((count + chunk - 1) / chunk) : 0, n_raw = results ? (size_t)count : 0;
	DevArray<char> d;
	StreamDrain drain{h->stream};
	HIP_TRY(h, d.alloc(n_fp * sizeof(uint64_t) + n_raw * sizeof(uint32_t)));
	unsigned long long *d_fp = n_fp ? (unsigned long long *)d.get() : nullptr;
	uint32_t *d_raw = n_raw ? (uint32_t *)(d + n_fp * sizeof(uint64_t)) : nullptr;
	if (n_fp) HIP_TRY(h, hipMemsetAsync(d_fp, 0, n_fp * sizeof(uint64_t), h->stream));
	const uint64_t span = (uint64_t)WG * kSweepPerThread, blocks = (count + span - 1) / span; // <= 2^32 / 4096
	hipLaunchKernelGGL(k_builtin_sweep, dim3((uint32_t)blocks), dim3(WG), 0, h->stream, fn, first, count, d_fp, d_raw);
	HIP_TRY(h, hipGetLastError());
	if (n_fp) HIP_TRY(h, hipMemcpyAsync(fingerprints, d_fp, n_fp * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
	if (n_raw) HIP_TRY(h, hipMemcpyAsync(results, d_raw, n_raw * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	return POLARIS_OK;
}

int polaris_hip_denoise_planes(polaris_hip_tracer *h, const float *acc, const float *guide, const float *albedo, uint32_t W, uint32_t H,
                               uint32_t block_y, uint32_t block_h, float weight, float exposure, const PolarisDenoiseParams *p,
                               float *denoised, uint8_t *rgba) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const char *rule = !acc || !guide || !albedo || !denoised || !rgba || !p ? plane_rule_text(kRuleNull) : frame_rows_rule(W, H, block_y, block_h);
	if (!rule && (p->struct_size != sizeof(PolarisDenoiseParams) || p->iterations == 0 || dn_check(p->iterations, p->normal_power_log2, p->sigma_depth, p->sigma_luminance)))
		rule = "params polaris_hip_set_denoise refuses, or iterations 0";
	if (rule) return refuse_planes(h, "denoise_planes", rule, W, H, block_y, block_h);
	return filter_planes_entry(h, SyncFeatures{true, false, false, false}, acc, guide, albedo, W, H, block_y, block_h, 0.0f, weight, exposure, *p, PolarisVarianceParams{},
	                           nullptr, denoised, rgba);
}

int polaris_hip_variance_planes(polaris_hip_tracer *h, const float *acc, const float *guide, const float *albedo, uint32_t W, uint32_t H,
                                uint32_t block_y, uint32_t block_h, uint32_t samples, float exposure, const PolarisDenoiseParams *p,
                                const PolarisVarianceParams *v, float *variance, float *denoised, uint8_t *rgba) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const char *rule = !acc || !guide || !albedo || !variance || !denoised || !rgba || !p || !v ? plane_rule_text(kRuleNull) : frame_rows_rule(W, H, block_y, block_h);
	if (!rule && (p->struct_size != sizeof(PolarisDenoiseParams) || v->struct_size != sizeof(PolarisVarianceParams) || samples == 0 ||
	              dn_check(p->iterations, p->normal_power_log2, p->sigma_depth, p->sigma_luminance) || v->sigma_variance == 0.0f || va_check(v->sigma_variance, v->min_samples)))
		rule = "samples 0, or params polaris_hip_set_denoise / _set_variance refuse, or sigma_variance 0";
	if (rule) return refuse_planes(h, "variance_planes", rule, W, H, block_y, block_h);
	const float weight = (float)(1.0 / (float)samples); // (polaris_hip_sync_framebuffer's)
	return filter_planes_entry(h, SyncFeatures{p->iterations != 0, false, true, false}, acc, guide, albedo, W, H, block_y, block_h, (float)samples, weight, exposure, *p, *v,
	                           variance, denoised, rgba);
}

int polaris_hip_display_planes(polaris_hip_tracer *h, const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight,
                               float exposure, const PolarisDisplayParams *p, const float *prev_log2E, uint8_t *rgba, uint32_t histogram[256],
                               PolarisExposureInfo *info) {
	return display_planes_entry(h, "display_planes", plane, W, H, block_y, block_h, weight, exposure, p, nullptr, false, prev_log2E, rgba, histogram, info, nullptr, nullptr);
}

int polaris_hip_bloom_planes(polaris_hip_tracer *h, const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight,
                             float exposure, const PolarisDisplayParams *dp, const PolarisBloomParams *bp, const float *prev_log2E, uint8_t *rgba,
                             float *level1, uint32_t *levels_used) {
	return display_planes_entry(h, "bloom_planes", plane, W, H, block_y, block_h, weight, exposure, dp, bp, true, prev_log2E, rgba, nullptr, nullptr, level1, levels_used);
}

int polaris_hip_reproject_planes(polaris_hip_tracer *h, const float *history, const float *prev_guide, const float *prev_albedo,
                                 const float prev_eye[3], const float prev_frustum[16], const float *guide, const float *albedo,
                                 const float eye[3], const float frustum[16], uint32_t W, uint32_t H, const PolarisTemporalParams *p,
                                 float *prior) {
	return reproject_planes_entry(h, "reproject_planes", ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, W, H, p, prior});
}

int polaris_hip_reproject_motion_planes(polaris_hip_tracer *h, const float *history, const float *prev_guide, const float *prev_albedo,
                                        const uint32_t *prev_instance, const float prev_eye[3], const float prev_frustum[16], const float *guide,
                                        const float *albedo, const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t W,
                                        uint32_t H, uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                        const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2) {
	return reproject_planes_entry(h, "reproject_motion_planes",
	                              ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, W, H, p, prior, kRpMotion, history_variance,
	                                          prior2, prev_instance, instance, n_instances, prev_inv_transforms, inv_transforms});
}

int polaris_hip_read_instance_plane(polaris_hip_tracer *h, uint32_t *out, size_t n) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const size_t need = (size_t)h->fa.W * h->fa.H;
	if (!out || n < need || need == 0) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_instance_plane: need %zu words", need);
	if (!h->fs.opt_object_motion) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_instance_plane: the option object_motion is off");
	HIP_TRY(h, hipSetDevice(h->device));
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
	if (!h->camera.have_camera) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_instance_plane: camera not set");
	if (!h->fs.features().motion_on()) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_instance_plane: object_motion has an effect only with temporal reuse on");
	if (int rc = ensure_gbuffer(h)) return rc;
	HIP_TRY(h, hipMemcpyAsync(out, h->fs.gb_inst, need * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	collect_timers(h);
	return POLARIS_OK;
}

int polaris_hip_reproject_deform_planes(polaris_hip_tracer *h, const float *history, const float *prev_guide, const float *prev_albedo,
                                        const uint32_t *prev_instance, const float prev_eye[3], const float prev_frustum[16], const float *guide,
                                        const float *albedo, const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t W,
                                        uint32_t H, uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                        const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2,
                                        const uint32_t *hit, const float *vertices, const float *prev_vertices, uint32_t num_triangles) {
	return reproject_planes_entry(h, "reproject_deform_planes",
	                              ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, W, H, p, prior, kRpDeform, history_variance,
	                                          prior2, prev_instance, instance, n_instances, prev_inv_transforms, inv_transforms, hit, vertices, prev_vertices, num_triangles});
}

int polaris_hip_read_hit_plane(polaris_hip_tracer *h, uint32_t *out, size_t n_words) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	const size_t need = 4 * (size_t)h->fa.W * h->fa.H;
	if (!out || n_words < need || need == 0) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_hit_plane: need %zu words", need);
	if (!h->fs.opt_vertex_motion) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_hit_plane: the option vertex_motion is off");
	HIP_TRY(h, hipSetDevice(h->device));
	if (!h->ds.have_scene) return fail(h, POLARIS_E_NO_SCENE_DATA, "no scene data uploaded");
	if (!h->camera.have_camera) return fail(h, POLARIS_E_BAD_ARGUMENT, "read_hit_plane: camera not set");
	if (!h->fs.features().deform_on())
		return fail(h, POLARIS_E_BAD_ARGUMENT, "read_hit_plane: vertex_motion has an effect only with object_motion in effect on a scene uploaded with vertex_update");
	if (int rc = ensure_gbuffer(h)) return rc;
	HIP_TRY(h, hipMemcpyAsync(out, h->fs.gb_hit, need * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	collect_timers(h);
	return POLARIS_OK;
}

int polaris_hip_kernel_symbol(polaris_hip_tracer *h, const char *kernel, char symbol[128]) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!kernel || !symbol) return fail(h, POLARIS_E_BAD_ARGUMENT, "kernel_symbol: null argument");
	auto it = h->timer_symbol.find(kernel);
	snprintf(symbol, 128, "%s", it == h->timer_symbol.end() ? "" : it->second);
	return POLARIS_OK;
}

int polaris_hip_shade_counts(polaris_hip_tracer *h, uint64_t *counts, size_t n_counts) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!counts || n_counts < 4 * (size_t)POLARIS_MAX_BOUNCES) return fail(h, POLARIS_E_BAD_ARGUMENT, "shade_counts: need 4 * POLARIS_MAX_BOUNCES entries");
	for (int b = 0; b < POLARIS_MAX_BOUNCES; b++) {
		counts[4 * b] = h->last_shade_counts[3 * b];
		counts[4 * b + 1] = h->last_shade_counts[3 * b + 1];
		counts[4 * b + 2] = h->last_shade_counts[3 * b + 2];
		counts[4 * b + 3] = (uint64_t)h->last_shade_timer[b];
	}
	return POLARIS_OK;
}

int polaris_hip_kernel_ms(polaris_hip_tracer *h, const char *kernel, double *ms, uint64_t *launches) {
	if (!h) return fail(nullptr, POLARIS_E_BAD_ARGUMENT, "handle is null");
	std::lock_guard<std::mutex> lk(h->mu);
	if (!kernel) return fail(h, POLARIS_E_BAD_ARGUMENT, "kernel name is null");
	auto it = h->timers.find(kernel);
	KernelTimer t = it == h->timers.end() ? KernelTimer{} : it->second;
	if (it != h->timers.end()) h->timers.erase(it);
	if (ms) *ms = t.ms;
	if (launches) *launches = t.launches;
	return POLARIS_OK;
}

} // extern "C"
