// bloom_plan_check.cpp -- test tap for what the bloom bit changes in frame_sync.h's plan of a sync (tests/test_bloom_cpu.py).
// bloom_plan() is plan_sync under one of the states of display_plan_check.cpp, restated here.  Everything travels as an int64: the
// features as bits (1 denoise, 2 temporal, 4 variance, 8 object motion, 16 vertex motion, 32 display, 64 auto-exposure, 128 bloom).
#include "frame_sync.h"

using namespace pol;

static SyncFeatures features_of(int64_t bits) {
	SyncFeatures f;
	f.denoise = bits & 1; f.temporal = bits & 2; f.variance = bits & 4; f.motion = bits & 8; f.deform = bits & 16;
	f.display = bits & 32; f.auto_exposure = bits & 64; f.bloom = bits & 128;
	return f;
}

// The states: 0 fresh; 1 a sync with every feature ran; 2 then the camera moved (a history with M2); 3 then PRIOR was computed;
// 4 as 2, then the vertices changed (the history has a snapshot); 5 as 3, then another sync ran.
static SyncState state_of(int64_t id) {
	SyncState v;
	SyncFeatures all;
	all.denoise = all.temporal = all.variance = all.motion = all.deform = true;
	if (id >= 1) { v.gbuffer_computed(); v.prior_computed(); v.synced(all); }
	if (id >= 2) (void)v.camera_moved(all);
	if (id == 3 || id == 5) { v.gbuffer_computed(); v.prior_computed(); }
	if (id == 4) (void)v.vertices_changing(all);
	if (id == 5) v.synced(all);
	return v;
}

extern "C" {

int64_t bloom_plan_states() { return 6; }
int64_t bloom_plan_max_steps() { return kMaxSyncSteps; }
int64_t bloom_plan_bloomed(int64_t features) { return features_of(features).bloomed(); }

// out[0..10]: the plan's head as display_plan_check.cpp's; out[11 ..]: kMaxSyncSteps steps, -1 past n_steps.
void bloom_plan(int64_t state, int64_t features, int64_t out[32]) {
	const SyncPlan p = plan_sync(features_of(features), state_of(state));
	const int64_t head[] = {p.need, p.clear, p.clear_new, p.prior, p.history, p.m2, p.motion, p.deform, (int64_t)p.color, (int64_t)p.tonemap, p.n_steps};
	for (int i = 0; i < 11; i++) out[i] = head[i];
	for (int i = 0; i < kMaxSyncSteps; i++) out[11 + i] = i < p.n_steps ? (int64_t)p.steps[i] : -1;
}

// plan_sync as it was before SyncFeatures had the bloom bit (it is not looked at), restated from the state's accessors alone.
void bloom_plan_before(int64_t state, int64_t features, int64_t out[32]) {
	const SyncFeatures f = features_of(features);
	const SyncState v = state_of(state);
	int64_t steps[kMaxSyncSteps];
	int n = 0;
	const int64_t need = planes(kGuide, kAlbedo) | (f.motion_on() ? planes(kInst) : 0) | (f.deform_on() ? planes(kHit) : 0) |
	                     (f.denoise ? planes(kDnOut, kDnPing, kDnPong) : 0) | (f.temporal ? planes(kTpOut, kTpPrior) : 0) | (f.variance ? planes(kVaOut) : 0) |
	                     (f.temporal && f.variance ? planes(kTpPrior2) : 0);
	int64_t clear = 0, clear_new = 0, prior = 0, history = 0, m2 = 0, motion = 0, deform = 0, color = (int64_t)SyncSource::Accumulator;
	if (f.temporal) {
		clear = (v.temporal_synced() ? 0 : planes(kTpOut)) | (f.variance && !v.variance_synced() ? planes(kVaOut) : 0);
		prior = !v.prior();
		history = prior && v.have_history();
		m2 = history && f.variance && v.history_has_m2();
		motion = history && f.motion;
		deform = motion && f.deform && v.history_has_snapshot();
		steps[n++] = (int64_t)SyncStep::Temporal;
		color = (int64_t)SyncSource::Temporal;
	} else if (f.variance) clear_new = planes(kVaOut);
	if (f.variance) steps[n++] = (int64_t)SyncStep::Variance;
	if (f.denoise) steps[n++] = (int64_t)(f.variance ? SyncStep::DenoiseVariance : SyncStep::Denoise);
	if (!f.display) steps[n++] = (int64_t)SyncStep::Tonemap;
	else {
		if (f.auto_exposure) { steps[n++] = (int64_t)SyncStep::Meter; steps[n++] = (int64_t)SyncStep::Expose; }
		steps[n++] = (int64_t)SyncStep::Display;
	}
	const int64_t head[] = {need, clear, clear_new, prior, history, m2, motion, deform, color, f.denoise ? (int64_t)SyncSource::Denoised : color, n};
	for (int i = 0; i < 11; i++) out[i] = head[i];
	for (int i = 0; i < kMaxSyncSteps; i++) out[11 + i] = i < n ? steps[i] : -1;
}

// plan_tail alone (the plain sync): out[0] = n, then the steps.
void bloom_plan_tail(int64_t features, int64_t out[8]) {
	SyncStep steps[kMaxSyncSteps];
	const int n = plan_tail(features_of(features), steps, 0);
	out[0] = n;
	for (int i = 0; i < kMaxSyncSteps; i++) out[1 + i] = i < n ? (int64_t)steps[i] : -1;
}
const char *bloom_plan_step_timer(int64_t step) { return kSyncStepTimer[step]; }

} // extern "C"
