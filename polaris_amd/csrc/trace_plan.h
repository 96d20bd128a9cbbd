// trace_plan.h -- what a Trace decides, as pure host functions over plain inputs: the batch size, the batches and pipelines, the
// kernels of every bounce, the grids of the persistent launches, and which traversal kernel traces a set of rays.
//
// No HIP here and no device code: polaris_hip.hip fills the inputs from the handle (the options ARE the handle's: TraceOptions is
// its member, written by polaris_hip_set_option), asks once per Trace and launches what the plan says; tests/tools/trace_plan_check.cpp
// asks the same functions on a CPU.  kernel_table.h cannot be read by a host compiler, so kernels are named by enum here and
// polaris_hip.hip maps the enums onto kPacket / kShade / kShadeWave.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "polaris_types.h"

namespace pol {

// The kernels' geometry the rules below count in.  kernels.h defines the kernels' own constants; polaris_hip.hip asserts these equal them.
constexpr uint32_t kPlanChunk = 256;      // slots of a chunk of rays == threads of a workgroup (WG)
constexpr uint32_t kPlanSparseGroup = 8;  // chunks a wave of k_shade_wave pulls at a time (kSparseGroup)
constexpr uint32_t kPlanTinyBlock = 1024; // threads of a k_trace workgroup in the tiny-scene mode (kTinyBlock)
constexpr int kMaxPipes = 8;              // pipelines a handle owns (option "overlap" is at most this)

// ---- the per-Trace options (polaris_hip_set_option clamps them; include/polaris_hip.h describes them)
struct TraceOptions {
	int64_t samples_per_batch = 0; // 0 = auto
	int exact = 0;
	int overlap = 4; // number of pipelines used (1 = no overlap)
	int packet_shadow = 0;   // shadow rays of the first N bounces go through the packet kernel too
	int packet_primary = -1; // wave-packet traversal (k_trace_packet) for bounce 0: 1/0, -1 = by scene size (TraceScene::packet_primary)
	int traversal = 1;       // 1 = persistent waves with lane refill (k_trace), 0 = one ray per lane (k_intersect/k_occlusion)
	int trace_wgs_per_cu = 0; // 0 = auto (what the LDS stack admits)
	int trace_grid = 0;       // 0 = auto; > 0: the persistent traversal grid in workgroups (A/B aid)
	int stage_lds = 1;    // k_shade stages material nodes / lights / texture metadata in LDS when they fit
	int shade_wave = 1;   // 1 = persistent wave-per-chunk shading (k_shade_wave), 0 = one workgroup per chunk (k_shade)
	int shade_wgs_per_cu = 0; // k_shade_wave's persistent grid in workgroups per CU; 0 = auto (what a CU holds of it: TraceScene::shade_wave_resident)
	int shade_wave_from = -1; // first bounce shaded by k_shade_wave; -1 = automatic (plan_shading): the bounce AFTER Russian roulette
	                          // starts thinning the chunks (min_bounces_for_rr + 1), or the roulette bounce itself where the prefilter
	                          // thins its chunks and the launch is large; earlier bounces use k_shade
	int shade_prefilter = 1; // the shade kernels retire rays that only count -- escaped, or rejected by Russian roulette off an emitter -- before shade_ray (kernels.h, shade_fate)
	int shade_sort = -1; // first bounce whose rays k_shade groups by shading class; -1 = default (1), POLARIS_MAX_BOUNCES = never
	int hit12 = 1;     // 12-byte hit records inside a Trace (A/B aid: 0 = 16)
	int o12 = 1;       // 12-byte origins of the closest-hit rays inside a Trace (A/B aid: 0 = 16)
};

// ---- what the plan needs to know of the uploaded scene and of the device
struct TraceScene {
	bool tiny = false;                // the tiny-scene mode (node mode kNodesLdsAll: two 1 024-thread workgroups fill a CU)
	int resident_per_cu[2] = {6, 6};  // [any hit]: workgroups of the scene's k_trace variant a CU holds at once
	bool tables_fit_lds = false;      // all three tables of the shade kernels fit their LDS copies (kernels.h, stage_scene)
	uint32_t emit_classes = 0;        // the shading classes that can end in an emitter (scene_layout.h, emitting_classes)
	uint32_t tri_bits = 0;            // 31: the hit word has no room for a shading class, nothing to sort by
	bool packet_primary = true;       // option packet_primary, resolved by the upload where it is -1
	int num_cus = 256;
	int shade_wave_resident[2] = {5, 5}; // [LDS tables]: workgroups of k_shade_wave<..> a CU holds at once (occupancy API: 5 waves per SIMD)
	bool lens = false;                // polaris_hip_set_lens is on: the camera rays start on the lens, each at its own origin
	bool shutter = false;             // polaris_hip_set_shutter is on: each camera ray starts at the eye of its own time; plans exactly as `lens`
	bool projection = false;          // polaris_hip_set_projection is on: the generator writes every ray's origin (the orthographic camera's differ); plans exactly as `lens`
};

// ---- which traversal kernel traces a set of rays
enum class RayKind { Camera, Closest, AnyHit }; // Camera: closest hit of a batch's camera rays, which share their origin (pinhole only, shutter off)
enum class Traversal { Packet, Persistent, Plain }; // k_trace_packet | the scene's k_trace variant | k_intersect / k_occlusion

inline Traversal traversal_unless_packet(bool packet, const TraceOptions &o) { return packet ? Traversal::Packet : (o.traversal ? Traversal::Persistent : Traversal::Plain); }
// The three entry points choose by different rules; each is kept as it was measured and tested.
// A batch: the packet kernel takes the camera rays where the upload resolved packet_primary, and the shadow rays of the first packet_shadow bounces.
inline Traversal batch_traversal(const TraceOptions &o, const TraceScene &s, RayKind kind, uint32_t bounce) {
	return traversal_unless_packet(kind == RayKind::AnyHit ? (int)bounce < o.packet_shadow : (bounce == 0 && s.packet_primary), o);
}
// polaris_hip_probe_intersect: the kernel the options select for bounce rays; only packet_primary = 1 (not the automatic choice) sends
// closest-hit probes through the wave-packet kernel.
inline Traversal probe_traversal(const TraceOptions &o, RayKind kind) {
	return traversal_unless_packet(kind == RayKind::AnyHit ? o.packet_shadow > 0 : o.packet_primary == 1, o);
}
// polaris_hip_tap_primary: the packet kernel or k_intersect, never k_trace.
inline Traversal tap_traversal(const TraceScene &s) { return s.packet_primary ? Traversal::Packet : Traversal::Plain; }
// The timer of a batch's traversal launch: one per kernel family of the closest-hit rays, one for the shadow rays.
inline const char *traversal_timer(Traversal how, RayKind kind) {
	return kind == RayKind::AnyHit ? "occlusion" : (how == Traversal::Packet ? "intersect_packet" : "intersect");
}
// A probe's persistent grid: what the GPU holds of the scene's k_trace variant at once, no more than there are chunks.
inline uint32_t probe_grid(const TraceScene &s, bool any_hit, uint32_t wgs) {
	return std::min<uint32_t>(wgs, (uint32_t)s.num_cus * (uint32_t)std::max(1, s.resident_per_cu[any_hit]));
}
// LDS-table variant of the shade kernels and of k_probe: only when all three tables fit.
inline bool tables_staged(const TraceOptions &o, const TraceScene &s) { return o.stage_lds && s.tables_fit_lds; }

// ---- the batch buffers
// Stream buffers per path slot: 128 B + one NEE record array per bounce (+ the per-chunk words); the NEE records are kept per bounce
// until the batch folds them.
inline size_t slot_bytes(uint32_t nee_bounces) { return 144 + 17 * (size_t)std::max(1u, nee_bounces); }
// Up to ~32 M paths per batch, but at least two batches so that one's sparse late bounces run beside the other's
// dense early ones.  Bigger batches amortise the tail of every persistent launch (a workgroup finishes the longest
// of its last rays alone) over more chunks -- measured on the round-2 kernels: headline frame 2 x 16.8 M paths
// 17.5 ms, 4 x 8.4 M 18.3 ms, 8 x 4.2 M 19.8 ms, 1 x 33.5 M 18.8 ms; 1024^2 x 256 spp: 33.5 M per batch 130.7 ms,
// 16.8 M 134.9 ms, 8.4 M 142.4 ms.  (128 B of stream buffers per path: 4.3 GB per batch in flight, of 288 GB.)
constexpr uint32_t kBatchPathBudget = 32u << 20;
constexpr int64_t kMaxSamplesPerBatch = 4096; // of a caller-chosen samples_per_batch
// Automatic shade_wave_from: a full batch must hold this many groups of kPlanSparseGroup chunks per CU for k_shade_wave to take the
// roulette bounce itself (profiles/shade_sparse_ab.txt).  The count is per CU, not per resident wave: at the
// threshold a launch fills half of the 16 waves a CU held when it was measured, and two fifths of the 20 it holds at five waves per
// SIMD (profiles/shade_wave_occupancy_ab.txt) -- it is the size below which k_shade's one workgroup per chunk was no slower, which the
// kernel's residency does not move.  (The headline frame's launches hold 32 groups per CU: 2 per wave at 16 waves, 1.6 at 20.)
constexpr uint32_t kWaveRouletteGroupsPerCu = 8;

// The shade kernel of a bounce, in the order of the shade timers (one timer per kernel symbol): k_shade<.., FIRST> (camera rays),
// k_shade<.., SORT, ..> (bounce rays in class order), k_shade<.., false, false>, k_shade_wave.
enum ShadeKernel { kShadeFirst, kShadeSort, kShadePlain, kShadeByWave };

// What one bounce of a Trace launches.
struct BouncePlan {
	Traversal isect = Traversal::Persistent, occl = Traversal::Persistent; // of its closest-hit / shadow rays
	ShadeKernel shade = kShadeFirst;
};

// Every input is fixed per Trace (options, request) or per upload: planned once, before the batches.  K alone may still shrink, by the
// free memory (clamp_to_memory) or after a failed allocation (shrink); whatever depends on it follows (set_batch).
struct TracePlan {
	TraceOptions opt;
	TraceScene scene;
	uint32_t spp = 0, bounces = 0, min_rr = 0, Npad = kPlanChunk;

	bool exact = false;      // one sample at a time into the trace accumulator, on one pipeline
	bool k_chosen = false;   // by the caller (samples_per_batch): kept as it is, an allocation's failure is reported
	uint32_t K = 1;          // samples per batch
	uint32_t n_batches = 0;
	int n_pipes = 1;         // pipelines used = batches in flight
	bool staged = false;     // the shade kernels' LDS-table variants
	bool moments = false, prefilter = true, hit12 = true, o12 = true; // the options the launches pass on
	bool generate_writes_origins = true; // (neither the wave-packet kernel nor k_trace's camera launch reads the origin stream)
	RayKind primary = RayKind::Camera;   // bounce 0's closest-hit rays; Closest under a lens, a shutter or a projection: the same kernel family, reading the origin stream
	BouncePlan bounce[POLARIS_MAX_BOUNCES];

	uint32_t pipes_wanted() const { return (uint32_t)std::max(1, std::min(opt.overlap, kMaxPipes)); }
	bool overlapping() const { return pipes_wanted() > 1 && !exact; } // several batches in flight share the CUs

	// K, and what follows from it: the batches, the pipelines and the shade kernels (the automatic shade_wave_from counts the chunks of a full batch).
	void set_batch(uint32_t k) {
		K = k;
		n_batches = spp ? (spp + K - 1) / K : 0;
		n_pipes = exact ? 1 : (int)std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)opt.overlap, n_batches));
		plan_shading();
	}

	// The batch buffers are slot_bytes per path slot and up to `overlap` batches are in flight: 4.3 GB per pipeline at 33.5 M slots,
	// nothing on a 288 GB MI355X but not on a smaller or shared device.  K chosen automatically is first clamped by the free device
	// memory (available = free + what the pipelines already hold; nine tenths of it) and, if an allocation still fails, halved and
	// retried (a caller-chosen samples_per_batch is kept as it is: its failure is reported).
	bool wants_memory_clamp() const { return !exact && !k_chosen && K > 1; }
	size_t bytes_needed(uint32_t k) const { // (batches in flight = min(overlap, #batches): it grows towards `overlap` as K shrinks)
		return (size_t)k * Npad * slot_bytes(bounces) * std::min<size_t>(pipes_wanted(), (spp + k - 1) / k);
	}
	void clamp_to_memory(size_t available) {
		if (!wants_memory_clamp()) return;
		const size_t budget = available / 10 * 9;
		uint32_t k = K;
		while (k > 1 && bytes_needed(k) > budget) k = (k + 1) / 2;
		set_batch(k);
	}
	// After an allocation failed for want of memory: the next smaller K; false: the failure is final.
	bool shrink() {
		if (exact || k_chosen || K == 1) return false;
		set_batch((K + 1) / 2);
		return true;
	}

	// Persistent traversal grid of a launch over `wgs` chunks (a tail batch is smaller than a full one): chunks are dealt to
	// workgroups statically, so a workgroup that is not resident from the start begins with its whole share still to do -- the grid
	// must not exceed what the GPU holds at once (measured: 8 workgroups per CU where 6 fit cost the closest-hit kernel 12 %).  One
	// batch at a time: exactly the resident capacity.  Several batches in flight: two thirds of it per launch (the launches share
	// the CUs; measured flat to +5 % across the bench scenes).
	// (LDS: 16-entry stack: 16 KB per workgroup -> 8 by LDS, VGPRs allow 7-8 waves/SIMD; 32-entry: 5)
	uint32_t trace_grid(bool any_hit, uint32_t wgs) const {
		uint32_t per_cu = (uint32_t)std::max(1, scene.resident_per_cu[any_hit]);
		if (overlapping() && per_cu > 2) per_cu = std::max(2u, per_cu * 2u / 3u);
		// tiny-scene mode (two 1 024-thread workgroups fill a CU), small launches -- a row block of a multi-GPU frame: with two
		// batches in flight a launch gets half the GPU at best, and at fewer than 4 chunks per resident wave a full-size grid
		// leaves every wave a single chunk, i.e. nothing but its ramp-down.  One workgroup per CU then: a 64-row block of the
		// headline frame 2.10 -> 1.83 ms, a 128-row block 3.30 -> 3.13 ms (256 rows +-0, the full frame +1 %: not applied there)
		if (scene.tiny && overlapping() && per_cu == 2 && (uint64_t)wgs < 4ull * (uint64_t)scene.num_cus * per_cu * (kPlanTinyBlock / 64))
			per_cu = 1;
		if (opt.trace_wgs_per_cu > 0) per_cu = (uint32_t)opt.trace_wgs_per_cu;
		if (opt.trace_grid > 0) return std::min<uint32_t>(wgs, (uint32_t)opt.trace_grid); // (A/B aid: an absolute persistent grid)
		return std::min<uint32_t>(wgs, (uint32_t)scene.num_cus * per_cu);
	}
	// k_shade_wave's grid: persistent waves pull groups of kPlanSparseGroup chunks: no more workgroups than the GPU holds at once (the
	// occupancy of the variant the plan launches, asked of the runtime: 5 per CU at the kernel's 96 registers) nor than there are
	// groups for their 4 waves -- and, below that, the FEWEST that leave no wave more groups than the full grid would: every wave then
	// takes the same number.  A group is ~100 us of dependent round trips and a launch holds one or two per wave, so the launch lasts
	// as long as its busiest wave: the headline frame's 8192 groups on all 5120 resident waves are two groups for three waves in five
	// and one for the rest -- measured no faster, on one card 0.1 ms per frame slower, than 4096 waves with two each
	// (profiles/shade_wave_occupancy_ab.txt), which is what this rule gives there (two rounds: 1024 workgroups), the registers the
	// fifth wave would hold left to the other batch's kernels.  Option shade_wgs_per_cu > 0 (A/B aid): that many per CU, as given.
	uint32_t shade_wave_grid(uint32_t wgs) const {
		const uint32_t groups = (wgs + kPlanSparseGroup - 1) / kPlanSparseGroup;
		if (opt.shade_wgs_per_cu > 0) return std::max(1u, std::min<uint32_t>((groups + 3) / 4, (uint32_t)scene.num_cus * (uint32_t)opt.shade_wgs_per_cu));
		const uint32_t waves = 4u * (uint32_t)scene.num_cus * (uint32_t)std::max(1, scene.shade_wave_resident[staged]); // resident at once
		const uint32_t rounds = std::max(1u, (groups + waves - 1) / waves); // groups of the busiest wave on the full grid
		return std::max(1u, (groups + 4u * rounds - 1) / (4u * rounds));
	}

private:
	void plan_shading() {
		// First bounce of k_shade_wave.  The bounce where Russian roulette starts still finds the chunks as the previous bounce left them;
		// only with the prefilter (shade_fate retires the rays roulette rejects, where some shading class cannot emit: otherwise nothing is
		// retired) does a chunk of that bounce hold a sixth of its rays, and k_shade still pays a workgroup's latency chain per chunk.
		// k_shade_wave screens and shades them a group at a time -- on launches large enough to keep its persistent grid busy: smaller
		// ones (a row block of a multi-GPU frame, the frames of the tests) keep the plan they had.
		int wave_from = opt.shade_wave_from;
		if (wave_from < 0) {
			wave_from = (int)min_rr + 1;
			const uint64_t batch_chunks = (uint64_t)K * (Npad / kPlanChunk); // the chunks of one full batch: the size of its shade launches
			const uint64_t groups = (batch_chunks + kPlanSparseGroup - 1) / kPlanSparseGroup;
			if (opt.shade_prefilter && (scene.emit_classes & 0xFFFFu) != 0xFFFFu && groups >= (uint64_t)kWaveRouletteGroupsPerCu * (uint64_t)scene.num_cus)
				wave_from = (int)min_rr;
		}
		for (uint32_t b = 0; b < bounces; b++) {
			const bool wave = opt.shade_wave && b > 0 && (int)b >= wave_from; // (never the first bounce: k_shade_wave reads the previous step's emit masks)
			// bounce rays are shaded in the order of their material's shading class (kernels.h, k_shade SORT); camera rays are
			// coherent as they come (64 neighbouring pixels per wave)
			const bool sorted = b > 0 && scene.tri_bits < 31 && (int)b >= (opt.shade_sort >= 0 ? opt.shade_sort : 1);
			bounce[b].shade = wave ? kShadeByWave : (b == 0 ? kShadeFirst : (sorted ? kShadeSort : kShadePlain));
		}
	}
};

// The plan of a Trace of `spp` samples of `Npad` path slots (a multiple of kPlanChunk, not 0) over `bounces` <= POLARIS_MAX_BOUNCES bounces.
inline TracePlan plan_trace(const TraceOptions &opt, const TraceScene &scene, bool moments, uint32_t spp, uint32_t bounces, uint32_t min_rr, uint32_t Npad) {
	TracePlan p;
	p.opt = opt; p.scene = scene;
	p.spp = spp; p.bounces = bounces; p.min_rr = min_rr; p.Npad = Npad;
	p.exact = opt.exact != 0;
	p.k_chosen = opt.samples_per_batch > 0;
	p.staged = tables_staged(opt, scene);
	p.moments = moments; p.prefilter = opt.shade_prefilter != 0; p.hit12 = opt.hit12 != 0; p.o12 = opt.o12 != 0;
	const bool own_origins = scene.lens || scene.shutter || scene.projection; // a generator that gives every camera ray its own origin
	p.generate_writes_origins = own_origins || !(bounces > 0 && (scene.packet_primary || opt.traversal));
	p.primary = own_origins ? RayKind::Closest : RayKind::Camera;
	for (uint32_t b = 0; b < bounces; b++) {
		p.bounce[b].isect = batch_traversal(opt, scene, b == 0 ? p.primary : RayKind::Closest, b);
		p.bounce[b].occl = batch_traversal(opt, scene, RayKind::AnyHit, b);
	}
	uint32_t K = 1;
	if (!p.exact) {
		if (p.k_chosen) K = (uint32_t)std::min<int64_t>(opt.samples_per_batch, kMaxSamplesPerBatch);
		else K = std::min<uint32_t>(std::max<uint32_t>(1u, kBatchPathBudget / Npad), std::max(1u, (spp + 1) / 2));
		K = std::max<uint32_t>(1u, std::min(K, std::max(spp, 1u)));
	}
	p.set_batch(K);
	return p;
}

} // namespace pol
