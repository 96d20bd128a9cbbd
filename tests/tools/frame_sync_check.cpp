// frame_sync_check.cpp -- test tap for frame_sync.h (tests/test_frame_sync_cpu.py): the validity state of the synced frame's planes,
// its transitions, the plan of a sync and the refusals of read_aov, on a CPU.  Everything travels as an int64: the features as bits
// (1 denoise, 2 temporal, 4 variance, 8 object motion), sets of planes as the header's bit masks.
#include "frame_sync.h"

using namespace pol;

static SyncFeatures features_of(int64_t bits) {
	SyncFeatures f;
	f.denoise = bits & 1; f.temporal = bits & 2; f.variance = bits & 4; f.motion = bits & 8;
	return f;
}

// The instance tables of the tests.  1: two instances of meshes 0 and 1; 2: the same instances moved; 3: another mesh in the second
// instance; 4: matrices only, as read back from the device; 5: what an upload with the option off passes (empty).
static InstTable table_of(int64_t id) {
	InstTable t;
	if (id == 5) return t;
	t.mesh_index = {0u, id == 3 ? 2u : 1u};
	t.inv.assign(32, id == 2 ? 2.0f : 1.0f);
	t.num_triangles = 10;
	t.topology_known = id != 4;
	if (id == 4) t.mesh_index = {0u, 0u};
	return t;
}

extern "C" {

void *frame_sync_new() { return new SyncState(); }
void frame_sync_delete(void *s) { delete (SyncState *)s; }

enum Event { Resized, CameraMoved, SceneChanged, TemporalParamsChanged, TemporalOff, VarianceToggled, MotionToggled, GbufferComputed, PriorComputed, Synced };

// One transition; returns the set of planes it hands the owner (to free, or for CameraMoved / SceneChanged to swap).
// arg: SceneChanged: the next table's id (0: none); VarianceToggled / MotionToggled: on.
int64_t frame_sync_event(void *s, int64_t event, int64_t features, int64_t arg) {
	SyncState &v = *(SyncState *)s;
	const SyncFeatures f = features_of(features);
	const InstTable next = table_of(arg);
	switch ((Event)event) {
	case Resized: return v.resized();
	case CameraMoved: return v.camera_moved(f);
	case SceneChanged: return v.scene_changed(f, arg ? &next : nullptr);
	case TemporalParamsChanged: v.temporal_params_changed(); return 0;
	case TemporalOff: return v.temporal_off();
	case VarianceToggled: return v.variance_toggled(arg != 0);
	case MotionToggled: return v.motion_toggled(arg != 0);
	case GbufferComputed: v.gbuffer_computed(); return 0;
	case PriorComputed: v.prior_computed(); return 0;
	case Synced: v.synced(f); return 0;
	}
	return -1;
}

// bits: 1 gbuffer, 2 prior, 4 have_history, 8 history_has_m2, 16 temporal_synced, 32 variance_synced
int64_t frame_sync_flags(const void *s) {
	const SyncState &v = *(const SyncState *)s;
	return v.gbuffer() | v.prior() << 1 | v.have_history() << 2 | v.history_has_m2() << 3 | v.temporal_synced() << 4 | v.variance_synced() << 5;
}

// which of the tables above the state's two tables equal (by mesh indices, matrices and topology flag); -1: neither of them
static int64_t table_id(const InstTable &t) {
	for (int64_t id = 1; id <= 5; id++) {
		const InstTable o = table_of(id);
		if (t.mesh_index == o.mesh_index && t.inv == o.inv && t.num_triangles == o.num_triangles && t.topology_known == o.topology_known) return id;
	}
	return -1;
}
int64_t frame_sync_table(const void *s, int64_t hist) { return table_id(hist ? ((const SyncState *)s)->hist : ((const SyncState *)s)->cur); }
void frame_sync_set_current_table(void *s, int64_t id) { ((SyncState *)s)->cur = table_of(id); } // (as the read-back after the option is turned on)

const char *frame_sync_aov_refusal(const void *s, int64_t which, int64_t temporal, int64_t have_prior2) {
	return ((const SyncState *)s)->aov_refusal((int)which, temporal != 0, have_prior2 != 0);
}

// out[0..12]: need, clear, clear_new, prior, history, m2, motion, color, tonemap, n_steps, steps[0..3] (-1 past n_steps)
void frame_sync_plan(const void *s, int64_t features, int64_t out[14]) {
	const SyncPlan p = plan_sync(features_of(features), *(const SyncState *)s);
	const int64_t head[] = {p.need, p.clear, p.clear_new, p.prior, p.history, p.m2, p.motion, (int64_t)p.color, (int64_t)p.tonemap, p.n_steps};
	for (int i = 0; i < 10; i++) out[i] = head[i];
	for (int i = 0; i < 4; i++) out[10 + i] = i < p.n_steps ? (int64_t)p.steps[i] : -1;
}
const char *frame_sync_step_timer(int64_t step) { return kSyncStepTimer[step]; }
int64_t frame_sync_plane_sets(int64_t which) {
	const uint32_t sets[] = {kDenoisePlanes, kTemporalPlanes, kVariancePlanes, kMomentPlanes, kMotionPlanes};
	return sets[which];
}

} // extern "C"
