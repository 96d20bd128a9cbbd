// display_plan_check.cpp -- test tap for what the display stage changes in frame_sync.h's plan of a sync
// (tests/test_display_cpu.py).  display_plan() is plan_sync under one of a few states; display_plan_before() is the plan as
// plan_sync made it before the display bits existed, restated here from the state's accessors alone, so that the bits off can be
// compared with it over every feature combination.  Everything travels as an int64: the features as bits (1 denoise, 2 temporal,
// 4 variance, 8 object motion, 16 vertex motion, 32 display, 64 auto-exposure).
#include "frame_sync.h"

using namespace pol;

static SyncFeatures features_of(int64_t bits) {
	SyncFeatures f;
	f.denoise = bits & 1; f.temporal = bits & 2; f.variance = bits & 4; f.motion = bits & 8; f.deform = bits & 16;
	f.display = bits & 32; f.auto_exposure = bits & 64;
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

static void put(const SyncPlan &p, int64_t out[18]) {
	const int64_t head[] = {p.need, p.clear, p.clear_new, p.prior, p.history, p.m2, p.motion, p.deform, (int64_t)p.color, (int64_t)p.tonemap, p.n_steps};
	for (int i = 0; i < 11; i++) out[i] = head[i];
	for (int i = 0; i < kMaxSyncSteps; i++) out[11 + i] = i < p.n_steps ? (int64_t)p.steps[i] : -1;
	out[17] = kMaxSyncSteps;
}

extern "C" {

int64_t display_plan_states() { return 6; }

void display_plan(int64_t state, int64_t features, int64_t out[18]) { put(plan_sync(features_of(features), state_of(state)), out); }

// plan_sync as it was before SyncFeatures had the display bits (they are not looked at).
void display_plan_before(int64_t state, int64_t features, int64_t out[18]) {
	const SyncFeatures f = features_of(features);
	const SyncState v = state_of(state);
	SyncPlan p;
	p.need = planes(kGuide, kAlbedo) | (f.motion_on() ? planes(kInst) : 0) | (f.deform_on() ? planes(kHit) : 0) | (f.denoise ? planes(kDnOut, kDnPing, kDnPong) : 0) |
	         (f.temporal ? planes(kTpOut, kTpPrior) : 0) | (f.variance ? planes(kVaOut) : 0) | (f.temporal && f.variance ? planes(kTpPrior2) : 0);
	if (f.temporal) {
		p.clear = (v.temporal_synced() ? 0 : planes(kTpOut)) | (f.variance && !v.variance_synced() ? planes(kVaOut) : 0);
		p.prior = !v.prior();
		p.history = p.prior && v.have_history();
		p.m2 = p.history && f.variance && v.history_has_m2();
		p.motion = p.history && f.motion;
		p.deform = p.motion && f.deform && v.history_has_snapshot();
		p.steps[p.n_steps++] = SyncStep::Temporal;
		p.color = SyncSource::Temporal;
	} else if (f.variance) p.clear_new = planes(kVaOut);
	if (f.variance) p.steps[p.n_steps++] = SyncStep::Variance;
	if (f.denoise) p.steps[p.n_steps++] = f.variance ? SyncStep::DenoiseVariance : SyncStep::Denoise;
	p.steps[p.n_steps++] = SyncStep::Tonemap;
	p.tonemap = f.denoise ? SyncSource::Denoised : p.color;
	put(p, out);
}

// plan_tail alone (the plain sync): out[0] = n, out[1..3] the steps.
void display_plan_tail(int64_t features, int64_t out[4]) {
	SyncStep steps[kMaxSyncSteps];
	const int n = plan_tail(features_of(features), steps, 0);
	out[0] = n;
	for (int i = 0; i < 3; i++) out[1 + i] = i < n ? (int64_t)steps[i] : -1;
}
const char *display_plan_step_timer(int64_t step) { return kSyncStepTimer[step]; }

} // extern "C"
