// vertex_motion_state_check.cpp -- a stand-alone program over frame_sync.h (tests/test_vertex_motion_cpu.py): the rule of the history's
// vertices (option "vertex_motion").  It drives a SyncState through the event sequences below as FrameSync and
// polaris_hip_update_vertices do in polaris_hip.hip and prints, per event, what the owner is told: the planes to swap or free, whether
// the vertex array is to be copied into the snapshot now, and what the next temporal sync's plan says.  Host code only.
#include <cstdio>
#include <cstring>

#include "frame_sync.h"

using namespace pol;

namespace {

struct Owner {
	SyncState v;
	SyncFeatures f;
	const char *seq;
	explicit Owner(const char *name, bool option = true) : seq(name) {
		f.temporal = f.motion = true;
		f.deform = option;
		InstTable t; // the upload: two instances of two meshes, the option "object_motion" on before it
		t.mesh_index = {0u, 1u};
		t.inv.assign(32, 1.0f);
		t.num_triangles = 10;
		t.topology_known = true;
		v.scene_changed(f, &t);
	}
	void say(const char *event, uint32_t planes, int snapshot) {
		printf("%s | %s | planes 0x%x | snapshot %d | history %d | has_snapshot %d\n", seq, event, planes, snapshot, (int)v.have_history(), (int)v.history_has_snapshot());
	}
	void sync() { // polaris_hip_sync_framebuffer with temporal reuse on
		const SyncPlan p = plan_sync(f, v);
		v.gbuffer_computed();
		if (p.prior) v.prior_computed();
		v.synced(f);
		printf("%s | sync | reads history %d | deform kernel %d | HIT plane %d\n", seq, (int)p.history, (int)p.deform, (int)(p.need >> kHit & 1));
	}
	void camera() { say("camera", v.camera_moved(f), 0); }
	void deform() { // polaris_hip_update_vertices
		if (!f.deform_on()) return say("deform", v.scene_changed(f, nullptr), 0);
		const InstTable next = v.cur;
		const uint32_t swaps = v.scene_changed(f, &next);
		say("deform", swaps, (int)v.vertices_changing(f));
	}
	void material() { say("material", v.scene_changed(f, nullptr), 0); } // polaris_hip_update_materials
	void option(bool on) { f.deform = on; say(on ? "option on" : "option off", v.deform_toggled(on), 0); }
	void resize() { say("resize", v.resized(), 0); }
};

} // namespace

int main() {
	{ Owner o("sync deform sync"); o.sync(); o.deform(); o.sync(); }
	{ Owner o("sync camera deform"); o.sync(); o.camera(); o.deform(); o.sync(); }
	{ Owner o("sync deform deform"); o.sync(); o.deform(); o.deform(); o.sync(); }
	{ Owner o("sync deform sync deform"); o.sync(); o.deform(); o.sync(); o.deform(); o.sync(); }
	{ Owner o("deform without history"); o.deform(); o.sync(); }
	{ Owner o("sync deform material"); o.sync(); o.deform(); o.material(); o.sync(); }
	{ Owner o("option toggled"); o.sync(); o.deform(); o.option(false); o.sync(); o.deform(); o.option(true); o.sync(); o.deform(); o.sync(); }
	{ Owner o("resize"); o.sync(); o.deform(); o.resize(); o.sync(); }
	{ Owner o("option off", false); o.sync(); o.deform(); o.sync(); }
	return 0;
}
