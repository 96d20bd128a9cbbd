// frame_sync.h -- the rules behind polaris_hip_sync_framebuffer's lazily allocated planes, as pure host code: what of them is valid
// (SyncState, whose only mutators are one named transition per event), what a sync with the features in force does (plan_sync) and
// whether an AOV can be read (SyncState::aov_refusal).
//
// No HIP here and no device pointer: FrameSync in polaris_hip.hip owns the planes and pairs every transition with the frees and
// swaps it returns; tests/tools/frame_sync_check.cpp asks the same functions on a CPU.  DESIGN.md sections 10-10d and 10k-10m describe the features.
#pragma once

#include <cstdint>
#include <vector>

#include "polaris_hip.h"

namespace pol {

// The frame-sized planes, and the motion table.  Up to kNumPlanes4 they are float4 planes (FrameSync::pl); sets of planes are bit masks.
enum Plane : uint32_t {
	// the first seven are what polaris_hip_read_aov reads, numbered as POLARIS_AOV_*: the first-hit G-buffer, DENOISED, TEMPORAL, PRIOR,
	// VARIANCE (M1 | M2 | n_eff | v) and PRIOR2 (h2 | 0 | 0 | m)
	kGuide, kAlbedo, kDnOut, kTpOut, kTpPrior, kVaOut, kTpPrior2,
	kDnPing, kDnPong,                        // the filter's iteration buffers
	kTpHist, kTpHGuide, kTpHAlbedo, kVaHist, // the history: TEMPORAL, the G-buffer and VARIANCE of the last temporal sync before the latest change
	kNumPlanes4,
	kInst = kNumPlanes4, kHInst,             // INSTANCE (one word per pixel, with object motion in effect), the history's
	kMoTable,                                // motion table of the last PRIOR (temporal.h tp_motion_table): not frame-sized, grow-only
	kHit,                                    // HIT (one uint4 per pixel, with vertex motion in effect): no history twin.  With it go the vertices the
	                                         // history was seen with and the deformation table, which are not frame-sized and grow only
};
static_assert(kGuide == POLARIS_AOV_GUIDE && kAlbedo == POLARIS_AOV_ALBEDO && kDnOut == POLARIS_AOV_DENOISED && kTpOut == POLARIS_AOV_TEMPORAL &&
              kTpPrior == POLARIS_AOV_PRIOR && kVaOut == POLARIS_AOV_VARIANCE && kTpPrior2 == POLARIS_AOV_PRIOR2, "read_aov reads plane `which`");
template <class... P> constexpr uint32_t planes(P... p) { return (0u | ... | (1u << p)); }
// Every plane is freed with exactly one of these sets.  kMomentPlanes exist only with temporal reuse AND variance guidance on and
// go when either goes; kMotionPlanes only with object motion in effect -- and kHit's, which exist only with vertex motion in effect,
// go with them or with kVertexMotionPlanes alone.
constexpr uint32_t kDenoisePlanes = planes(kGuide, kAlbedo, kDnOut, kDnPing, kDnPong), kMomentPlanes = planes(kVaHist, kTpPrior2),
                   kMotionPlanes = planes(kInst, kHInst, kMoTable), kVertexMotionPlanes = planes(kHit), kVariancePlanes = planes(kVaOut),
                   kTemporalPlanes = planes(kTpOut, kTpPrior, kTpHist, kTpHGuide, kTpHAlbedo) | kMotionPlanes | kMomentPlanes;

// The instance table a scene was seen with (option "object_motion"): a host copy made by an upload with the option on.  Turned on after
// the upload, the matrices are read back from the device's instance records; the mesh indices are not there: compatible with nothing.
struct InstTable {
	std::vector<uint32_t> mesh_index;
	std::vector<float> inv; // 16 floats of inv_transform per instance
	uint32_t num_triangles = 0;
	bool topology_known = false; // mesh_index and num_triangles are the scene's
	bool compatible(const InstTable &o) const {
		return topology_known && o.topology_known && mesh_index == o.mesh_index && num_triangles == o.num_triangles;
	}
};

// The features in force at an event.  motion: the option "object_motion"; it is in effect only with temporal reuse on.  deform: the
// option "vertex_motion" on a scene uploaded with "vertex_update"; it is in effect only with object motion in effect.
struct SyncFeatures {
	bool denoise = false, temporal = false, variance = false, motion = false, deform = false;
	bool display = false, auto_exposure = false; // polaris_hip_set_display: the sync's last step is the display stage, metered or not
	bool bloom = false;                          // polaris_hip_set_bloom: in effect only with the display stage on
	bool any() const { return denoise || temporal || variance; }
	bool motion_on() const { return motion && temporal; }
	bool deform_on() const { return deform && motion_on(); }
	bool metered() const { return display && auto_exposure; }
	bool bloomed() const { return display && bloom; }
};

class SyncState {
	bool gb_valid = false;       // the G-buffer is computed for the current scene, camera and frame size
	bool dn_valid = false;       // a denoised sync has written DENOISED since the last resize
	bool tp_have_hist = false;   // the history planes hold a history
	bool tp_synced = false;      // a temporal sync ran under the current camera (TEMPORAL and the G-buffer are this camera's)
	bool tp_prior_valid = false; // PRIOR is the current history reprojected into the current camera with the current params
	bool va_valid = false;       // a variance sync has written VARIANCE (under the current camera with temporal reuse)
	bool va_synced = false;      // temporal: a variance sync ran under the current camera (VARIANCE is this camera's)
	bool va_have_hist = false;   // temporal: the history has a VARIANCE plane (its M2)
	bool hist_verts_current = true; // vertex motion: the history was seen with the vertices the device holds now (no snapshot is needed)

	// Nothing synced so far was seen under what holds from now on: the camera or the scene.
	void forget_syncs() { tp_synced = tp_prior_valid = va_synced = va_valid = false; }
	// The last temporal sync's planes under the current camera and scene become the history; no such sync: the older history stays.
	// Returns the planes to swap with their history twin (kTpOut, kGuide and kAlbedo together; kInst; kVaOut).  The VARIANCE plane
	// joins the history only if it was written under the same camera; else the history has no M2.
	uint32_t capture_history(bool motion_on) {
		if (!tp_synced) return 0;
		tp_have_hist = true;
		va_have_hist = va_synced;
		if (motion_on) hist = cur;
		hist_verts_current = true; // (the sync that joins the history ran under the scene as it is)
		return planes(kTpOut, kGuide, kAlbedo) | (motion_on ? planes(kInst) : 0) | (va_synced ? planes(kVaOut) : 0);
	}

public:
	InstTable cur, hist; // the current scene's instance table and the history's (kept with the option "object_motion" only)

	bool gbuffer() const { return gb_valid; }
	bool prior() const { return tp_prior_valid; }
	bool have_history() const { return tp_have_hist; }       bool history_has_m2() const { return va_have_hist; }
	bool history_has_snapshot() const { return tp_have_hist && !hist_verts_current; } // (a dropped history forgets its snapshot)
	bool temporal_synced() const { return tp_synced; }       bool variance_synced() const { return va_synced; }

	// ---- the transitions.  Those that return a set of planes: the owner frees them (or swaps them, where it says so).
	uint32_t resized() { // every plane is frame-sized (a plane exists only under its feature, so all of them go)
		gb_valid = dn_valid = tp_have_hist = tp_synced = tp_prior_valid = va_valid = va_synced = va_have_hist = false;
		return kDenoisePlanes | kTemporalPlanes | kVariancePlanes;
	}
	uint32_t camera_moved(const SyncFeatures &f) { // returns the planes to swap (capture_history)
		const uint32_t swaps = f.temporal ? capture_history(f.motion_on()) : 0;
		if (f.temporal) forget_syncs();
		gb_valid = false;
		return swaps;
	}
	// The scene changes (an upload or an in-place update, before it happens).  next: the instance table of the scene to come, which
	// becomes `cur`.  With object motion the change is to the history what a camera move is: the planes synced under the old scene join
	// it, and it survives if the scene to come has the same instances of the same meshes.  Otherwise, and always with next = null
	// (`cur` stays), the history saw another scene and goes.  Returns the planes to swap (capture_history).
	uint32_t scene_changed(const SyncFeatures &f, const InstTable *next) {
		gb_valid = false;
		uint32_t swaps = 0;
		bool keep = false;
		if (next && f.motion_on()) {
			swaps = capture_history(true);
			keep = tp_have_hist && hist.compatible(*next);
		}
		if (f.temporal) {
			if (!keep) tp_have_hist = va_have_hist = false;
			forget_syncs();
		}
		if (next) cur = *next;
		return swaps;
	}
	// polaris_hip_update_vertices with vertex motion in effect, after its scene_changed(f, next) and just before it overwrites the vertex
	// array: true -> the owner copies the array into the snapshot first (a history exists that was seen with it).  false: there is no
	// history, or it was seen with older vertices, whose snapshot stays (two deformations without a temporal sync in between).
	bool vertices_changing(const SyncFeatures &f) {
		if (!f.deform_on() || !tp_have_hist || !hist_verts_current) return false;
		hist_verts_current = false;
		return true;
	}
	void temporal_params_changed() { tp_prior_valid = false; } // (PRIOR is recomputed at the next temporal sync)
	uint32_t temporal_off() { tp_have_hist = tp_synced = tp_prior_valid = va_synced = va_have_hist = false; return kTemporalPlanes; }
	uint32_t variance_toggled(bool on) { // (PRIOR2 is written, or no longer, by the next temporal sync's reprojection)
		tp_prior_valid = false;
		if (!on) va_valid = va_synced = va_have_hist = false;
		return on ? 0 : kVariancePlanes | kMomentPlanes;
	}
	uint32_t motion_toggled(bool on) { // the history (with or without an INSTANCE plane) and the G-buffer go with the old setting
		guide_rule_changed();
		cur = hist = InstTable();
		return on ? 0 : kMotionPlanes;
	}
	uint32_t deform_toggled(bool on) { // (option "vertex_motion", or an upload that puts it in or out of effect) as motion_toggled; the instance table stays
		guide_rule_changed();
		return on ? 0 : kVertexMotionPlanes;
	}
	void guide_rule_changed() { // (option "guide_specular") the G-buffer and a history seen with the other rule go; the planes and the instance table stay
		tp_have_hist = tp_synced = tp_prior_valid = va_synced = va_have_hist = va_valid = gb_valid = false;
	}
	void gbuffer_computed() { gb_valid = true; }
	void prior_computed() { tp_prior_valid = true; }
	void synced(const SyncFeatures &f) { // a sync with these features completed
		if (f.temporal) tp_synced = true;
		if (f.temporal && f.variance) va_synced = true;
		if (f.denoise) dn_valid = true;
		if (f.variance) va_valid = true;
	}

	// Why polaris_hip_read_aov refuses POLARIS_AOV_<which> now; null: it can be read (GUIDE and ALBEDO are computed on demand).
	// have_prior2: the PRIOR2 plane exists.
	const char *aov_refusal(int which, bool temporal, bool have_prior2) const {
		if (which == POLARIS_AOV_DENOISED && !dn_valid) return "read_aov: no denoised sync since the last resize";
		if ((which == POLARIS_AOV_TEMPORAL || which == POLARIS_AOV_PRIOR) && (!tp_synced || !tp_prior_valid)) return "read_aov: no temporal sync under the current camera";
		if (which == POLARIS_AOV_VARIANCE && !va_valid) return temporal ? "read_aov: no variance sync under the current camera" : "read_aov: no variance sync since the last resize";
		if (which == POLARIS_AOV_PRIOR2 && (!va_valid || !temporal || !have_prior2)) return "read_aov: no variance sync with temporal reuse under the current camera";
		return nullptr;
	}
};

// ---- what a sync with features f does under state v (f.any(); the plain sync is plan_tail's steps over the accumulator and asks nothing)
enum class SyncSource { Accumulator, Temporal, Denoised }; // the accumulator is read with the sync's weight, the other two with weight 1
enum class SyncStep { Temporal, Variance, Denoise, DenoiseVariance, Tonemap, Meter, Expose, Display, Bloom };
constexpr const char *kSyncStepTimer[] = {"temporal", "variance", "denoise", "denoise_variance", "tonemap", "meter", "expose", "display", "bloom"}; // one timer per kernel symbol (denoise and bloom: one around their launches)
constexpr int kMaxSyncSteps = 7; // temporal, variance, a filter and the display stage's four
struct SyncPlan {
	uint32_t need = 0;      // planes that must exist (allocated on first use)
	uint32_t clear = 0;     // of those, cleared first: the rows no sync under this camera reaches must read as "no history"
	uint32_t clear_new = 0; // of those, cleared when this sync allocates them
	bool prior = false;     // PRIOR is stale: recomputed from the history (none: cleared) by kReproject[m2][motion]
	bool history = false, m2 = false, motion = false;
	bool deform = false;    // the history has a snapshot of the vertices: kReprojectDeform[m2] in kReproject's place
	SyncStep steps[kMaxSyncSteps] = {}; // the timed steps in launch order
	int n_steps = 0;
	SyncSource color = SyncSource::Accumulator, tonemap = SyncSource::Accumulator; // what the filter reads | what the tone-map reads (the filter's output, or its input where none runs)
};
// The steps that turn the sync's source into bytes, appended to steps[n]: the tone-map, or with the display stage on
// Meter and Expose (auto-exposure), Bloom (behind Expose: its bright pass reads the exposure) and Display.  They read
// no plane of their own: the histogram, the exposure state and the bloom pyramid belong to the display stage's owner.  The plain sync
// (no other feature) runs these steps alone.
inline int plan_tail(const SyncFeatures &f, SyncStep *steps, int n) {
	if (!f.display) steps[n++] = SyncStep::Tonemap;
	else {
		if (f.auto_exposure) { steps[n++] = SyncStep::Meter; steps[n++] = SyncStep::Expose; }
		if (f.bloom) steps[n++] = SyncStep::Bloom;
		steps[n++] = SyncStep::Display;
	}
	return n;
}
inline SyncPlan plan_sync(const SyncFeatures &f, const SyncState &v) {
	SyncPlan p;
	p.need = planes(kGuide, kAlbedo) | (f.motion_on() ? planes(kInst) : 0) | (f.deform_on() ? planes(kHit) : 0) | (f.denoise ? planes(kDnOut, kDnPing, kDnPong) : 0) |
	         (f.temporal ? planes(kTpOut, kTpPrior) : 0) | (f.variance ? planes(kVaOut) : 0) | (f.temporal && f.variance ? planes(kTpPrior2) : 0);
	if (f.temporal) {
		p.clear = (v.temporal_synced() ? 0 : planes(kTpOut)) | (f.variance && !v.variance_synced() ? planes(kVaOut) : 0);
		p.prior = !v.prior();
		p.history = p.prior && v.have_history();
		p.m2 = p.history && f.variance && v.history_has_m2();
		p.motion = p.history && f.motion; // (a history kept with object motion on has an INSTANCE plane and a table of the scene's size)
		p.deform = p.motion && f.deform && v.history_has_snapshot();
		p.steps[p.n_steps++] = SyncStep::Temporal;
		p.color = SyncSource::Temporal;
	} else if (f.variance) p.clear_new = planes(kVaOut);
	if (f.variance) p.steps[p.n_steps++] = SyncStep::Variance;
	if (f.denoise) p.steps[p.n_steps++] = f.variance ? SyncStep::DenoiseVariance : SyncStep::Denoise;
	p.n_steps = plan_tail(f, p.steps, p.n_steps);
	p.tonemap = f.denoise ? SyncSource::Denoised : p.color;
	return p;
}

} // namespace pol
