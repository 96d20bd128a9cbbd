// vertex_update_check.cpp -- CPU harness over polaris_amd/csrc/vertex_update.h (test tool, not product).
//
// vu_layout: the records build_layout makes of a scene, and the padding it gives the boxes leaf subdivision adds below every mesh.
// vu_update: build_layout of a base scene with the mesh plan, then the host restatement of polaris_hip_update_vertices (argument
// checks, triangle records, mesh refit, per-instance records, re-padding, top-level refit) applied to those records, in the
// library's order.  tests/test_vertex_update_cpu.py compares the second with the first run on the refit scene.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -Iinclude -Ipolaris_amd/csrc vertex_update_check.cpp
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "vertex_update.h"

using namespace pol;

namespace {

int say(char *err, size_t err_len, const std::string &e) {
	if (err && err_len) { strncpy(err, e.c_str(), err_len - 1); err[err_len - 1] = 0; }
	return 1;
}

std::string layout_of(const PolarisSceneView &sc, int max_leaf_tris, bool plan, SceneLayout &L) {
	L = SceneLayout();
	L.want_mesh_plan = plan;
	std::string e = build_layout(sc, L, max_leaf_tris);
	if (e == "@retry-without-subdivision") { L = SceneLayout(); L.want_mesh_plan = plan; e = build_layout(sc, L, 0); }
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

// The mesh plan names what it says it names: children before parents and on earlier levels, every node where its parent's record
// refers to it, every leaf with the slots the kernels see, one root per mesh.
std::string check_mesh_plan(const SceneLayout &L, uint32_t NN) {
	const MeshPlan &M = L.plan.mesh;
	if (M.level_first.empty() || M.level_first.front() != 0 || M.level_first.back() != M.nodes.size() || M.nodes.empty()) return "mesh plan: levels do not tile the nodes";
	if (M.slot_src.size() != L.tris.size()) return "mesh plan: slot_src does not cover the triangle slots";
	for (size_t s = 0; s < M.slot_src.size(); s++)
		if ((L.tris[s].orig & (L.tri_bits < 31 ? (1u << L.tri_bits) - 1u : ~0u)) != M.slot_src[s]) return "mesh plan: slot_src disagrees with the triangle records";
	std::vector<uint32_t> level_of(M.nodes.size());
	for (size_t l = 0; l + 1 < M.level_first.size(); l++)
		for (uint32_t i = M.level_first[l]; i < M.level_first[l + 1]; i++) level_of[i] = (uint32_t)l;
	size_t roots = 0;
	for (size_t i = 0; i < M.nodes.size(); i++) {
		const MeshPlanNode &u = M.nodes[i];
		if (u.mesh >= M.root.size()) return "mesh plan: bad mesh";
		int32_t ref;
		if (u.count && u.b < 0) {
			if (u.b != -1 || (uint64_t)(uint32_t)u.a + u.count > L.tris.size()) return "mesh plan: bad leaf";
			if (level_of[i] != 0) return "mesh plan: a leaf above the first level";
			ref = u.count <= 15 ? ~(int32_t)((uint32_t)u.a << 4 | u.count) : ~(int32_t)(kBigLeafFlag | u.node << 4);
			if (u.count > 15 && ((uint32_t)(-(int64_t)L.leaves[u.node].ldata) != (uint32_t)u.a || (uint32_t)L.leaves[u.node].rdata != u.count)) return "mesh plan: LeafInfo disagrees";
		} else {
			if (u.a < 0 || u.b < 0 || (size_t)u.a >= i || (size_t)u.b >= i || level_of[u.a] >= level_of[i] || level_of[u.b] >= level_of[i]) return "mesh plan: children do not come before their parent";
			if (M.nodes[u.a].pair_side != (M.nodes[u.b].pair_side ^ 1) || (M.nodes[u.a].pair_side & 1)) return "mesh plan: the children do not share one record";
			ref = M.nodes[u.a].pair_side >> 1;
			if (u.count && (u.node >= NN || (uint64_t)u.first_tri + u.count > L.tris.size())) return "mesh plan: bad split leaf";
		}
		if ((u.padded >= 0) != (u.node >= NN)) return "mesh plan: added nodes and padded boxes disagree";
		if (u.padded >= 0) {
			if ((size_t)u.padded >= L.plan.padded.size()) return "mesh plan: bad padded index";
			const PaddedBox &b = L.plan.padded[u.padded];
			if (b.pair != (u.pair_side >> 1) || b.side_mesh != ((uint32_t)(u.pair_side & 1) | u.mesh << 1)) return "mesh plan: the padded box is another node's";
		}
		if (u.pair_side < 0) {
			if (M.root[u.mesh] != i) return "mesh plan: a node without a parent is not its mesh's root";
			roots++;
			continue;
		}
		if ((size_t)(u.pair_side >> 1) >= L.pairs.size()) return "mesh plan: bad pair record";
		const PairNodeH &N = L.pairs[u.pair_side >> 1];
		if ((u.pair_side & 1 ? N.ref1 : N.ref0) != ref) return "mesh plan: the parent's record does not refer to node " + std::to_string(u.node);
	}
	if (roots != M.root.size()) return "mesh plan: not one root per mesh";
	return "";
}

} // namespace

extern "C" {

// pads (may be null): per distinct mesh root, in the order of the first instance that uses it, the padding build_layout gives the
// boxes it adds below that root (its own expression: the largest subdivision_pad over the mesh's instances).
int vu_layout(const PolarisSceneView *sc, int max_leaf_tris, void *pairs, void *insts, void *tris, size_t cap, uint32_t *counts, float *pads, uint32_t pads_cap,
              char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*sc, max_leaf_tris, false, L);
	if (!e.empty()) return say(err, err_len, e);
	if (pads) {
		std::vector<uint32_t> roots;
		for (uint32_t i = 0; i < sc->num_mesh_instances; i++) {
			const uint32_t root = sc->mesh_instances[i].bvh_root;
			size_t m = 0;
			while (m < roots.size() && roots[m] != root) m++;
			if (m == roots.size()) { roots.push_back(root); if (m < pads_cap) pads[m] = 0.0f; }
			if (m >= pads_cap) return say(err, err_len, "pads buffer too small");
			const float pad = subdivision_pad(sc->mesh_instances[i].inv_transform, sc->bvh_nodes[0], sc->bvh_nodes[root]);
			if (pad > pads[m]) pads[m] = pad;
		}
	}
	return copy_out(L, pairs, insts, tris, cap, counts, err, err_len);
}

// status: what polaris_hip_update_vertices would return (0, or the refusal: the records are then build_layout(base)'s, untouched).
// plan_sizes: mesh plan nodes, levels, meshes, padded boxes, 1 if a mesh plan was kept.  plan_nodes: the MeshPlanNode entries (32 bytes
// each), slot_src, padded: the PaddedBox entries (32 bytes each) after the update, pads: the update's padding per mesh.
int vu_update(const PolarisSceneView *base, int max_leaf_tris, int option_on, const PolarisVertexUpdate *u, void *pairs, void *insts, void *tris, size_t cap,
              uint32_t *counts, int *status, uint32_t *plan_sizes, void *plan_nodes, uint32_t *slot_src, void *padded, float *pads_out, char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*base, max_leaf_tris, option_on != 0, L);
	if (!e.empty()) return say(err, err_len, e);
	const MeshPlan &M = L.plan.mesh;
	if (M.on) {
		const std::string pe = check_mesh_plan(L, base->num_bvh_nodes);
		if (!pe.empty()) return say(err, err_len, pe);
	}
	plan_sizes[0] = (uint32_t)M.nodes.size(); plan_sizes[1] = (uint32_t)(M.level_first.empty() ? 0 : M.level_first.size() - 1);
	plan_sizes[2] = (uint32_t)L.plan.mesh_box.size(); plan_sizes[3] = (uint32_t)L.plan.padded.size(); plan_sizes[4] = M.on ? 1u : 0u;
	if (M.nodes.size() * sizeof(MeshPlanNode) > cap || M.slot_src.size() * 4 > cap || L.plan.padded.size() * sizeof(PaddedBox) > cap) return say(err, err_len, "output buffers too small");
	std::string msg;
	const std::vector<PolarisEmissive> ems(base->emissives, base->emissives + base->num_emissives);
	const uint32_t NI = base->num_mesh_instances;
	std::vector<float> kept((size_t)NI * 16);
	for (uint32_t i = 0; i < NI; i++) memcpy(kept.data() + 16 * (size_t)i, base->mesh_instances[i].inv_transform, 64);
	*status = check_vertex_update(u, true, option_on != 0, M, base->num_triangles, NI, ems, msg);
	if (*status == 0) *status = check_vertex_magnitudes(u->vertices, base->num_triangles, msg);
	std::vector<InstUpdateRec> recs;
	std::vector<float> pads;
	const float *inv = *status == 0 && u->inv_transforms ? u->inv_transforms : kept.data();
	if (*status == 0) *status = prepare_instance_update(L.plan, NI, inv, u->instance_boxes, recs, pads, msg);
	if (*status == 0) {
		host_refit_mesh(L.plan, u->vertices, L.tris.data(), L.pairs.data());
		*status = prepare_instance_update(L.plan, NI, inv, u->instance_boxes, recs, pads, msg);
		host_refit(L.plan, recs, pads, u->vertices, L.pairs.data(), L.insts.data());
		memcpy(pads_out, pads.data(), pads.size() * sizeof(float));
	} else say(err, err_len, msg);
	memcpy(plan_nodes, M.nodes.data(), M.nodes.size() * sizeof(MeshPlanNode));
	memcpy(slot_src, M.slot_src.data(), M.slot_src.size() * 4);
	memcpy(padded, L.plan.padded.data(), L.plan.padded.size() * sizeof(PaddedBox));
	return copy_out(L, pairs, insts, tris, cap, counts, err, err_len);
}
}
