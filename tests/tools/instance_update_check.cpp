// instance_update_check.cpp -- CPU harness over polaris_amd/csrc/instance_update.h (test tool, not product).
//
// iu_layout: the records build_layout makes of a scene.  iu_update: build_layout of a base scene with the update plan, then the host
// restatement of polaris_hip_update_instances (argument checks, per-instance records, re-padding, refit, cull factors) applied to
// those records.  tests/test_instance_update_cpu.py asserts that the second equals the first run on the refit scene, byte for byte.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -Iinclude -Ipolaris_amd/csrc instance_update_check.cpp
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "instance_update.h"

using namespace pol;

namespace {

int say(char *err, size_t err_len, const std::string &e) {
	if (err && err_len) { strncpy(err, e.c_str(), err_len - 1); err[err_len - 1] = 0; }
	return 1;
}

std::string layout_of(const PolarisSceneView &sc, int max_leaf_tris, bool plan, SceneLayout &L) {
	L = SceneLayout();
	L.want_update_plan = plan;
	std::string e = build_layout(sc, L, max_leaf_tris);
	if (e == "@retry-without-subdivision") { L = SceneLayout(); L.want_update_plan = plan; e = build_layout(sc, L, 0); }
	return e;
}

// counts: pair, instance and triangle records
int copy_out(const SceneLayout &L, void *pairs, void *insts, void *tris, size_t cap, uint32_t *counts, char *err, size_t err_len) {
	counts[0] = (uint32_t)L.pairs.size(); counts[1] = (uint32_t)L.insts.size(); counts[2] = (uint32_t)L.tris.size();
	if (L.pairs.size() * sizeof(PairNodeH) > cap || L.insts.size() * sizeof(InstH) > cap || L.tris.size() * sizeof(TriH) > cap) return say(err, err_len, "output buffers too small");
	memcpy(pairs, L.pairs.data(), L.pairs.size() * sizeof(PairNodeH));
	memcpy(insts, L.insts.data(), L.insts.size() * sizeof(InstH));
	memcpy(tris, L.tris.data(), L.tris.size() * sizeof(TriH));
	return 0;
}

// The plan names the records it says it names: every node sits where its parent's record refers to it.
std::string check_plan(const SceneLayout &L) {
	const UpdatePlan &P = L.plan;
	if (P.level_first.empty() || P.level_first.back() != P.nodes.size() || P.nodes.empty()) return "plan: levels do not tile the nodes";
	uint32_t leaves = 0;
	for (size_t i = 0; i < P.nodes.size(); i++) {
		const UpdateNode &u = P.nodes[i];
		int32_t ref;
		if (u.pair < 0) {
			if (u.kid0 < 0 || (size_t)u.kid0 >= L.insts.size() || u.kid1 != -1) return "plan: bad leaf";
			ref = ~(int32_t)((uint32_t)u.kid0 << 4);
			leaves++;
		} else {
			if ((size_t)u.pair >= L.pairs.size() || u.kid0 < 0 || u.kid1 < 0 || (size_t)u.kid0 >= i || (size_t)u.kid1 >= i) return "plan: children do not come before their parent";
			ref = u.pair;
		}
		if (u.parent_side < 0) {
			if (i + 1 != P.nodes.size() || ref != L.root_ref) return "plan: the root is not the last node";
			continue;
		}
		const UpdateNode &up = P.nodes[(size_t)(u.parent_side >> 1)];
		if (up.pair < 0 || (u.parent_side & 1 ? up.kid1 : up.kid0) != (int32_t)i) return "plan: parent and child disagree";
		const PairNodeH &N = L.pairs[up.pair];
		if ((u.parent_side & 1 ? N.ref1 : N.ref0) != ref) return "plan: the parent's record does not refer to node " + std::to_string(i);
	}
	if (leaves != L.insts.size()) return "plan: not one leaf per instance";
	for (size_t l = 0; l + 1 < P.level_first.size(); l++) // a node's children are on earlier levels
		for (uint32_t i = P.level_first[l]; i < P.level_first[l + 1]; i++)
			if (P.nodes[i].pair >= 0 && ((uint32_t)P.nodes[i].kid0 >= P.level_first[l] || (uint32_t)P.nodes[i].kid1 >= P.level_first[l])) return "plan: a child on its parent's level";
	return "";
}

} // namespace

extern "C" {

int iu_layout(const PolarisSceneView *sc, int max_leaf_tris, void *pairs, void *insts, void *tris, size_t cap, uint32_t *counts, char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*sc, max_leaf_tris, false, L);
	if (!e.empty()) return say(err, err_len, e);
	return copy_out(L, pairs, insts, tris, cap, counts, err, err_len);
}

// status: what polaris_hip_update_instances would return (0, or the refusal: the records are then build_layout(base)'s, untouched).
// plan_sizes (may be null): plan nodes, levels, meshes, listed triangles, padded boxes.
int iu_update(const PolarisSceneView *base, int max_leaf_tris, int option_on, const PolarisInstanceUpdate *u, void *pairs, void *insts, void *tris, size_t cap,
              uint32_t *counts, int *status, uint32_t *plan_sizes, char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*base, max_leaf_tris, option_on != 0, L);
	if (!e.empty()) return say(err, err_len, e);
	if (option_on) {
		const std::string pe = check_plan(L);
		if (!pe.empty()) return say(err, err_len, pe);
	}
	if (plan_sizes) {
		plan_sizes[0] = (uint32_t)L.plan.nodes.size(); plan_sizes[1] = (uint32_t)(L.plan.level_first.empty() ? 0 : L.plan.level_first.size() - 1);
		plan_sizes[2] = (uint32_t)L.plan.mesh_box.size(); plan_sizes[3] = (uint32_t)L.plan.tri_list.size(); plan_sizes[4] = (uint32_t)L.plan.padded.size();
	}
	std::string msg;
	const std::vector<PolarisEmissive> ems(base->emissives, base->emissives + base->num_emissives);
	*status = check_instance_update(u, true, option_on != 0, base->num_mesh_instances, ems, msg);
	std::vector<InstUpdateRec> recs;
	std::vector<float> pads;
	if (*status == 0) *status = prepare_instance_update(L.plan, base->num_mesh_instances, u->inv_transforms, u->instance_boxes, recs, pads, msg);
	if (*status == 0) host_refit(L.plan, recs, pads, base->vertices, L.pairs.data(), L.insts.data());
	else say(err, err_len, msg);
	return copy_out(L, pairs, insts, tris, cap, counts, err, err_len);
}
}
