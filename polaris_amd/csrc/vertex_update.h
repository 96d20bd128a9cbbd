// vertex_update.h -- deforming meshes in place: polaris_hip_update_vertices.
//
// When only vertex positions change, the topology of every tree, the ranks, the stack depth, the slot order, the shading classes and
// the kernel variants of the uploaded scene stay; what changes is the vertex (and normal) arrays, the Tri records, the boxes the
// MESH-LEVEL pair records hold, the unpadded bounds of the boxes leaf subdivision added, every instance's world extent and the
// top-level boxes.  The update recomputes the first three on the device from the mesh plan build_layout kept (scene_layout.h,
// MeshPlan) and then runs the instance update's kernels (instance_update.h) for the rest:
//
//   k_tri_records  one thread per triangle slot: v0, v1 - v0, v2 - v0 of the slot's scene triangle, one IEEE subtraction each
//                  (build_layout's expression); the three .w words (rank, scene triangle | class, tiny meta word) stay.
//   k_refit_mesh   one thread per node of the mesh plan, a level at a time, leaves first: a leaf folds the vertices of its
//                  triangles (read from the vertex array through slot_src, in the leaf's own order, v0, v1, v2), an inner node
//                  unions its children's bounds, left before right.  (A leaf of the caller's tree that leaf subdivision split
//                  folds its scene triangles in the caller's order: the slots below it were sorted, and where +0 meets -0 the
//                  order decides the sign.)  The bounds go to a scratch array for the level above and to
//                  where the node's box is held: a node of the caller's tree writes box and cull factor 1.001 into its side of its
//                  parent's pair record (the box IS its content); a node leaf subdivision added writes its exact bounds into the
//                  device's PaddedBox entry, from which k_repad makes the padded box; a mesh root writes a per-mesh array, which the
//                  host reads back (the root's box is a term of the padding).
//
// The min / max rule is refit_inner's: b < a ? b : a and b > a ? b : a with a the running value, so where +0 meets -0 the earlier
// operand stays -- numpy (scenes.refit_vertices), the host and the device agree on the byte.
//
// The per-node arithmetic is __host__ __device__: host_refit_mesh below is the same code on the CPU, and
// tests/tools/vertex_update_check.cpp shows it byte-equal to build_layout of the refit scene.
#pragma once

#include "instance_update.h"

namespace pol {

constexpr uint32_t kTriRecordBlock = 256;
constexpr uint32_t kMeshRefitOneGroupNodes = 1024; // plans up to this many nodes are refit by ONE workgroup looping over the levels

// The floats of a triangle record: build_layout's expression.
POL_HD inline void tri_record(const float *v0, const float *v1, const float *v2, float *o_v0, float *o_e1, float *o_e2) {
	for (int k = 0; k < 3; k++) { o_v0[k] = v0[k]; o_e1[k] = v1[k] - v0[k]; o_e2[k] = v2[k] - v0[k]; }
}

// The running bounds with one more point folded in.
POL_HD inline void fold_point(float *lo, float *hi, const float *p) {
	for (int k = 0; k < 3; k++) {
		lo[k] = p[k] < lo[k] ? p[k] : lo[k];
		hi[k] = p[k] > hi[k] ? p[k] : hi[k];
	}
}

// Exact bounds of a leaf: its triangles in its own order, of each v0, v1, v2.  vertices: [3 NT][4]; count >= 1.  slot_src: the
// triangles are the slots [first, first + count); null: the scene triangles [first, first + count) themselves.
POL_HD inline void mesh_leaf_bounds(const float *vertices, const uint32_t *slot_src, uint32_t first, uint32_t count, float *lo, float *hi) {
	for (uint32_t s = first; s < first + count; s++) {
		const float *v = vertices + 4 * (size_t)(3 * (size_t)(slot_src ? slot_src[s] : s));
		if (s == first)
			for (int k = 0; k < 3; k++) lo[k] = hi[k] = v[k];
		else fold_point(lo, hi, v);
		fold_point(lo, hi, v + 4);
		fold_point(lo, hi, v + 8);
	}
}

// Bounds of an inner node: the left child's with the right child's folded in.
POL_HD inline void mesh_inner_bounds(const float *alo, const float *ahi, const float *blo, const float *bhi, float *lo, float *hi) {
	for (int k = 0; k < 3; k++) {
		lo[k] = blo[k] < alo[k] ? blo[k] : alo[k];
		hi[k] = bhi[k] > ahi[k] ? bhi[k] : ahi[k];
	}
}

// ---- host: the argument checks of polaris_hip_update_vertices that need no device ------------------------------------------------------
// have_plan: the scene was uploaded with the option vertex_update on; M: its mesh plan; NT, NI, ems: the uploaded scene's counts and
// emissive list.  0 = accepted, else the POLARIS_E_* status the entry returns, with msg.
inline int check_vertex_update(const PolarisVertexUpdate *u, bool have_scene, bool have_plan, const MeshPlan &M, uint32_t NT, uint32_t NI,
                               const std::vector<PolarisEmissive> &ems, std::string &msg) {
	if (!u) { msg = "vertex update is null"; return POLARIS_E_BAD_ARGUMENT; }
	if (!have_scene) { msg = "no scene data uploaded"; return POLARIS_E_NO_SCENE_DATA; }
	if (!have_plan) { msg = "update_vertices: the scene was uploaded with the option vertex_update off"; return POLARIS_E_UNSUPPORTED; }
	if (!M.on) { msg = "update_vertices: no mesh plan was kept: " + M.refused; return POLARIS_E_UNSUPPORTED; }
	if (u->struct_size != sizeof(PolarisVertexUpdate)) { msg = "update_vertices: struct_size is not sizeof(PolarisVertexUpdate)"; return POLARIS_E_BAD_ARGUMENT; }
	if (u->num_triangles != NT) {
		msg = "update_vertices: " + std::to_string(u->num_triangles) + " triangles, the uploaded scene has " + std::to_string(NT);
		return POLARIS_E_BAD_ARGUMENT;
	}
	if (u->num_mesh_instances != NI) {
		msg = "update_vertices: " + std::to_string(u->num_mesh_instances) + " mesh instances, the uploaded scene has " + std::to_string(NI);
		return POLARIS_E_BAD_ARGUMENT;
	}
	if (!u->vertices || !u->instance_boxes) { msg = "update_vertices: vertex or box pointer is null"; return POLARIS_E_BAD_ARGUMENT; }
	return check_update_emissives("update_vertices: ", u->emissives, u->num_emissives, ems, msg);
}

// build_layout's magnitude rule over the new vertices, with its text.
inline int check_vertex_magnitudes(const float *vertices, uint32_t NT, std::string &msg) {
	for (size_t i = 0; i < (size_t)NT * 3; i++) {
		const float *v = vertices + 4 * i;
		for (int k = 0; k < 3; k++)
			if (!(std::fabs(v[k]) <= kMaxCoordinate)) {
				msg = "triangle " + std::to_string(i / 3) + ": vertex coordinate not finite or beyond 2^40";
				return POLARIS_E_BAD_SCENE;
			}
	}
	return 0;
}

// ---- host: the restatement of the two kernels (test tools; the library runs the kernels) ------------------------------------------
// vertices: the NEW [3 NT][4]; tris / pairs: build_layout's records of the uploaded scene, refit in place; P.padded (the unpadded
// bounds) and P.mesh_box follow, as the device's copies do.  host_refit (instance_update.h) comes next, as in the library.
inline void host_refit_mesh(UpdatePlan &P, const float *vertices, TriH *tris, PairNodeH *pairs) {
	const MeshPlan &M = P.mesh;
	for (size_t s = 0; s < M.slot_src.size(); s++) {
		const float *v = vertices + 4 * (size_t)(3 * (size_t)M.slot_src[s]);
		tri_record(v, v + 4, v + 8, tris[s].v0, tris[s].e1, tris[s].e2);
	}
	struct Bounds { float lo[3], hi[3]; };
	std::vector<Bounds> scratch(M.nodes.size());
	for (size_t i = 0; i < M.nodes.size(); i++) { // (levels in order: children come before their parent)
		const MeshPlanNode &u = M.nodes[i];
		Bounds &me = scratch[i];
		if (u.count) mesh_leaf_bounds(vertices, u.b < 0 ? M.slot_src.data() : nullptr, u.b < 0 ? (uint32_t)u.a : u.first_tri, u.count, me.lo, me.hi);
		else mesh_inner_bounds(scratch[u.a].lo, scratch[u.a].hi, scratch[u.b].lo, scratch[u.b].hi, me.lo, me.hi);
		if (u.padded >= 0) {
			memcpy(P.padded[u.padded].lo, me.lo, 12);
			memcpy(P.padded[u.padded].hi, me.hi, 12);
		} else if (u.pair_side >= 0) {
			PairNodeH &N = pairs[u.pair_side >> 1];
			const float f = kCullMargin;
			memcpy(u.pair_side & 1 ? N.lo1 : N.lo0, me.lo, 12);
			memcpy(u.pair_side & 1 ? N.hi1 : N.hi0, me.hi, 12);
			memcpy(u.pair_side & 1 ? &N.pad1 : &N.pad0, &f, 4);
		} else {
			memcpy(P.mesh_box[u.mesh].min, me.lo, 12);
			memcpy(P.mesh_box[u.mesh].max, me.hi, 12);
		}
	}
}

#if defined(__HIPCC__)
// ---- device ---------------------------------------------------------------------------------------------------------------------------

// One thread per triangle slot.  The record's three 16-byte words are read for their .w and written whole.
__global__ __launch_bounds__(kTriRecordBlock) void k_tri_records(const float4 *__restrict__ vertices, const uint32_t *__restrict__ slot_src, uint32_t num_slots,
                                                                 TriRec *tris) {
	const uint32_t s = blockIdx.x * kTriRecordBlock + threadIdx.x;
	if (s >= num_slots) return;
	const float4 *v = vertices + 3ull * slot_src[s];
	const float4 a = v[0], b = v[1], c = v[2];
	const float p0[3] = {a.x, a.y, a.z}, p1[3] = {b.x, b.y, b.z}, p2[3] = {c.x, c.y, c.z};
	float v0[3], e1[3], e2[3];
	tri_record(p0, p1, p2, v0, e1, e2);
	TriRec *T = tris + s;
	const float w0 = T->v0.w, w1 = T->e1.w, w2 = T->e2.w;
	T->v0 = make_float4(v0[0], v0[1], v0[2], w0);
	T->e1 = make_float4(e1[0], e1[1], e1[2], w1);
	T->e2 = make_float4(e2[0], e2[1], e2[2], w2);
}

struct MeshRefitArgs {
	const MeshPlanNode *nodes;
	const uint32_t *level_first;
	const uint32_t *slot_src;
	const float4 *vertices;
	float4 *scratch;    // [plan nodes][2]: lo | 0, hi | 0
	PairNode *pairs;
	PaddedBox *padded;  // the device's copy of UpdatePlan::padded: k_repad reads the unpadded bounds there
	float4 *mesh_box;   // [meshes][2]
};

// Levels [level0, level0 + num_levels) of the mesh plan, one thread per node of a level.  More than one level: ONE workgroup, which
// loops over them (a level reads what the level before wrote: workgroup barrier in between); one level: any grid.  No two threads
// write the same 16-byte word: a node owns its scratch entry, its side of its parent's record, its PaddedBox entry or its mesh's box.
__global__ __launch_bounds__(kRefitBlock) void k_refit_mesh(MeshRefitArgs A, uint32_t level0, uint32_t num_levels) {
	for (uint32_t l = level0; l < level0 + num_levels; l++) {
		const uint32_t end = A.level_first[l + 1];
		for (uint32_t i = A.level_first[l] + blockIdx.x * kRefitBlock + threadIdx.x; i < end; i += gridDim.x * kRefitBlock) {
			const int4 w0 = reinterpret_cast<const int4 *>(A.nodes + i)[0], w1 = reinterpret_cast<const int4 *>(A.nodes + i)[1];
			const MeshPlanNode u{w0.x, w0.y, (uint32_t)w0.z, w0.w, w1.x, (uint32_t)w1.y, (uint32_t)w1.z, (uint32_t)w1.w};
			float lo[3], hi[3];
			if (u.count) mesh_leaf_bounds(reinterpret_cast<const float *>(A.vertices), u.b < 0 ? A.slot_src : nullptr, u.b < 0 ? (uint32_t)u.a : u.first_tri, u.count, lo, hi);
			else {
				const float4 alo = A.scratch[2 * (size_t)u.a], ahi = A.scratch[2 * (size_t)u.a + 1], blo = A.scratch[2 * (size_t)u.b], bhi = A.scratch[2 * (size_t)u.b + 1];
				const float al[3] = {alo.x, alo.y, alo.z}, ah[3] = {ahi.x, ahi.y, ahi.z}, bl[3] = {blo.x, blo.y, blo.z}, bh[3] = {bhi.x, bhi.y, bhi.z};
				mesh_inner_bounds(al, ah, bl, bh, lo, hi);
			}
			A.scratch[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], 0.0f);
			A.scratch[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
			if (u.padded >= 0) { // {pair, side | mesh << 1, lo.xy} {lo.z, hi.xyz}: the first two words are what the upload wrote
				float4 *d = reinterpret_cast<float4 *>(A.padded + u.padded);
				d[0] = make_float4(__int_as_float(u.pair_side >> 1), __uint_as_float((uint32_t)(u.pair_side & 1) | u.mesh << 1), lo[0], lo[1]);
				d[1] = make_float4(lo[2], hi[0], hi[1], hi[2]);
			} else if (u.pair_side >= 0) { // (.w of lo: the child reference stays)
				PairNode *N = A.pairs + (u.pair_side >> 1);
				float4 *plo = u.pair_side & 1 ? &N->lo1 : &N->lo0, *phi = u.pair_side & 1 ? &N->hi1 : &N->hi0;
				const float ref = __int_as_float(reinterpret_cast<const int4 *>(plo)->w);
				*plo = make_float4(lo[0], lo[1], lo[2], ref);
				*phi = make_float4(hi[0], hi[1], hi[2], kCullMargin);
			} else {
				A.mesh_box[2 * (size_t)u.mesh] = make_float4(lo[0], lo[1], lo[2], 0.0f);
				A.mesh_box[2 * (size_t)u.mesh + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
			}
		}
		if (num_levels > 1) { __threadfence_block(); __syncthreads(); }
	}
}
#endif // __HIPCC__

} // namespace pol
