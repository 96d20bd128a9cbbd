// instance_update.h -- moving mesh instances in place: polaris_hip_update_instances.
//
// When only instance matrices change, the mesh trees, the triangle records, the ranks, the stack depth and the kernel variants of
// the uploaded scene stay; what changes is the Inst records (rows of the inverse matrix) and the boxes and cull factors held in
// the TOP-LEVEL pair records.  The update refits those on the device from the plan build_layout kept (scene_layout.h, UpdatePlan):
//
//   k_instance_extent  per instance, the exact world extent of its mesh: every vertex of every triangle below its mesh root
//                      through the forward matrix, (float)(fwd[4r] * p0 + fwd[4r + 1] * p1 + fwd[4r + 2] * p2 + fwd[4r + 3]) in
//                      double, left to right, no contraction -- build_layout's own expression; min / max per workgroup (wave
//                      shuffles, then LDS), one partial box per (instance, chunk).  Min and max do not depend on the order.
//   k_repad            one thread per box that leaf subdivision added below a mesh root: the box with the padding a full upload
//                      would give it now (the padding depends on the instance matrices and the world box).
//   k_refit_top        one thread per node of the plan, a level at a time, deepest first: a leaf takes the caller's box
//                      verbatim, folds its instance's partial extents and writes Inst.r0..r2; an inner node takes the union
//                      of its children's boxes and contents and writes both children's lo / hi and cull factors into its pair record.
//
// The triangle records are not touched, so neither are the shading classes that ride in their `orig` words, and the material
// table does not change: SceneT::emit_classes (the classes that can end in an emitter, scene_layout.h) stays what the upload set.
//
// The per-node arithmetic (refit_leaf, refit_inner) is __host__ __device__: host_refit below is the same code on the CPU, and
// tests/tools/instance_update_check.cpp shows it byte-equal to build_layout of the refit scene.
//
// Deviation from a full upload: the device always takes the exact path, with all vertices.  build_layout falls back to the eight
// corners of the mesh's box beyond its work cap (32 M / 3 vertex transforms per upload), a superset -- above the cap it may give
// a child the factor +inf where the update gives 1.001.  Invisible in results: a factor is 1.001 only where the box really bounds
// its content, i.e. where culling is legal.
#pragma once

#include "polaris_hip.h"
#include "scene_layout.h"
#if defined(__HIPCC__)
#include "kernels.h"
#endif

namespace pol {

// What the host hands the kernels per instance and update.
struct InstUpdateRec {
	double fwd[12];             // forward matrix, rows 0-2, row major (invert_instance_matrix)
	float r0[4], r1[4], r2[4];  // rows of the inverse: what the Inst record takes
	float box[6];               // the caller's world box of the instance: min.xyz, max.xyz
	uint32_t valid;             // 0: singular matrix -- nothing can be promised about the instance's extent
	uint32_t pad;
};
static_assert(sizeof(InstUpdateRec) == 176, "layout");

// Box and content (real extent of everything below) of a plan node: the scratch record the levels hand upwards.
struct alignas(16) UpdateBox { float blo[3], bhi[3], clo[3], chi[3]; };
static_assert(sizeof(UpdateBox) == 48, "layout");

constexpr float kEmptyLo = 3.0e38f, kEmptyHi = -3.0e38f; // build_layout's empty box
constexpr uint32_t kExtentBlock = 256;        // threads of a k_instance_extent workgroup
constexpr uint32_t kExtentChunkTris = 2048;   // triangles per chunk, at least (8 per thread)
constexpr uint32_t kExtentMaxChunks = 256;    // chunks per instance, at most (a leaf thread of k_refit_top folds them)
constexpr uint32_t kRefitBlock = 256;
constexpr uint32_t kRefitOneGroupNodes = 1024; // plans up to this many nodes are refit by ONE workgroup looping over the levels

POL_HD inline void refit_leaf(const InstUpdateRec &R, const float *ext_lo, const float *ext_hi, UpdateBox &out) {
	for (int k = 0; k < 3; k++) {
		out.blo[k] = R.box[k];
		out.bhi[k] = R.box[3 + k];
		out.clo[k] = R.valid ? ext_lo[k] : -3.0e38f;
		out.chi[k] = R.valid ? ext_hi[k] : 3.0e38f;
	}
}

// Union of the children a (left) and b (right); f0 / f1: the cull factors of a and b in the parent's pair record.
// Boxes: component-wise min / max (fmin / fmax of finite values; a tie between +0 and -0 keeps the left child's).
// Contents: build_layout's merge, fmin / fmax over the left box and the right one's two corners.
POL_HD inline void refit_inner(const UpdateBox &a, const UpdateBox &b, UpdateBox &out, float &f0, float &f1) {
	for (int k = 0; k < 3; k++) {
		out.blo[k] = b.blo[k] < a.blo[k] ? b.blo[k] : a.blo[k];
		out.bhi[k] = b.bhi[k] > a.bhi[k] ? b.bhi[k] : a.bhi[k];
		out.clo[k] = fminf(fminf(a.clo[k], b.clo[k]), b.chi[k]);
		out.chi[k] = fmaxf(fmaxf(a.chi[k], b.clo[k]), b.chi[k]);
	}
	const float inf = __builtin_huge_valf();
	f0 = box_bounds_content(a.blo, a.bhi, a.clo, a.chi) ? kCullMargin : inf;
	f1 = box_bounds_content(b.blo, b.bhi, b.clo, b.chi) ? kCullMargin : inf;
}

// An added box with its padding: build_layout's expression.
POL_HD inline void repad_box(const PaddedBox &b, float pad, float *lo, float *hi) {
	for (int k = 0; k < 3; k++) { lo[k] = b.lo[k] - pad; hi[k] = b.hi[k] + pad; }
}

// One vertex through a forward matrix: build_layout's `world`.
POL_HD inline void world_point(const double *fwd, const float *v, float *w) {
	const double p[3] = {v[0], v[1], v[2]};
	for (int r = 0; r < 3; r++) w[r] = (float)(fwd[4 * r] * p[0] + fwd[4 * r + 1] * p[1] + fwd[4 * r + 2] * p[2] + fwd[4 * r + 3]);
}

// An update's emissive list (null: unchanged) may differ from the uploaded one (ems) in transform and area only.  who: the entry, for msg.
inline int check_update_emissives(const char *who, const PolarisEmissive *list, uint32_t n, const std::vector<PolarisEmissive> &ems, std::string &msg) {
	if (list && n != ems.size()) {
		msg = who + std::to_string(n) + " emissives, the uploaded scene has " + std::to_string(ems.size());
		return POLARIS_E_BAD_ARGUMENT;
	}
	for (uint32_t e = 0; list && e < n; e++)
		if (list[e].type != ems[e].type || list[e].tri_index != ems[e].tri_index || list[e].mat_node_index != ems[e].mat_node_index) {
			msg = who + ("emissive " + std::to_string(e)) + " differs from the uploaded one in type, triangle or material node";
			return POLARIS_E_BAD_ARGUMENT;
		}
	return 0;
}

// ---- host: the argument checks of polaris_hip_update_instances that need no device ----------------------------------------------------
// have_plan: the scene was uploaded with the option instance_update on; NI, ems: the uploaded scene's instance count and emissive
// list.  0 = accepted, else the POLARIS_E_* status the entry returns, with msg.
inline int check_instance_update(const PolarisInstanceUpdate *u, bool have_scene, bool have_plan, uint32_t NI, const std::vector<PolarisEmissive> &ems,
                                 std::string &msg) {
	if (!u) { msg = "instance update is null"; return POLARIS_E_BAD_ARGUMENT; }
	if (!have_scene) { msg = "no scene data uploaded"; return POLARIS_E_NO_SCENE_DATA; }
	if (!have_plan) { msg = "update_instances: the scene was uploaded with the option instance_update off"; return POLARIS_E_UNSUPPORTED; }
	if (u->struct_size != sizeof(PolarisInstanceUpdate)) { msg = "update_instances: struct_size is not sizeof(PolarisInstanceUpdate)"; return POLARIS_E_BAD_ARGUMENT; }
	if (u->num_mesh_instances != NI) {
		msg = "update_instances: " + std::to_string(u->num_mesh_instances) + " mesh instances, the uploaded scene has " + std::to_string(NI);
		return POLARIS_E_BAD_ARGUMENT;
	}
	if (!u->inv_transforms || !u->instance_boxes) { msg = "update_instances: matrix or box pointer is null"; return POLARIS_E_BAD_ARGUMENT; }
	return check_update_emissives("update_instances: ", u->emissives, u->num_emissives, ems, msg);
}

// ---- host: validation and the per-instance records ------------------------------------------------------------------------------
// status: 0 = accepted, else POLARIS_E_BAD_SCENE; msg says why.  inv: [NI][16] column major; boxes: [NI][6].
// pads: per mesh of the plan, the padding of the boxes leaf subdivision added below its root.
inline int prepare_instance_update(const UpdatePlan &P, uint32_t NI, const float *inv, const float *boxes, std::vector<InstUpdateRec> &recs,
                                   std::vector<float> &pads, std::string &msg) {
	for (uint32_t i = 0; i < NI; i++) {
		for (int k = 0; k < 16; k++)
			if (!(std::fabs(inv[16 * (size_t)i + k]) <= kMaxMatrixEntry)) {
				msg = "mesh instance " + std::to_string(i) + ": matrix entry not finite or beyond 2^30";
				return POLARIS_E_BAD_SCENE;
			}
		const float *b = boxes + 6 * (size_t)i;
		for (int k = 0; k < 3; k++)
			if (!(std::fabs(b[k]) <= std::numeric_limits<float>::max() && std::fabs(b[3 + k]) <= std::numeric_limits<float>::max() && b[k] <= b[3 + k])) {
				msg = "mesh instance " + std::to_string(i) + ": box not finite or min > max";
				return POLARIS_E_BAD_SCENE;
			}
	}
	// the padding of the boxes leaf subdivision added, as a full upload computes it: from the refit world box (the root's box =
	// the min / max over every instance box) and the new matrices, the largest over a mesh's instances
	PolarisBvhNode world{};
	for (int k = 0; k < 3; k++) { world.min[k] = boxes[k]; world.max[k] = boxes[3 + k]; }
	for (uint32_t i = 1; i < NI; i++)
		for (int k = 0; k < 3; k++) {
			world.min[k] = std::fmin(world.min[k], boxes[6 * (size_t)i + k]);
			world.max[k] = std::fmax(world.max[k], boxes[6 * (size_t)i + 3 + k]);
		}
	pads.assign(P.mesh_box.size(), 0.0f);
	for (uint32_t i = 0; i < NI; i++) {
		const uint32_t m = P.mesh_of_inst[i];
		const float pad = subdivision_pad(inv + 16 * (size_t)i, world, P.mesh_box[m]);
		if (pad > pads[m]) pads[m] = pad;
	}
	recs.assign(NI, InstUpdateRec{});
	for (uint32_t i = 0; i < NI; i++) {
		InstUpdateRec &R = recs[i];
		const float *m = inv + 16 * (size_t)i; // column major: m[4 * c + r]
		double fwd[16];
		R.valid = invert_instance_matrix(m, fwd) ? 1u : 0u;
		for (int k = 0; k < 12; k++) R.fwd[k] = R.valid ? fwd[k] : 0.0;
		for (int c = 0; c < 4; c++) { R.r0[c] = m[4 * c + 0]; R.r1[c] = m[4 * c + 1]; R.r2[c] = m[4 * c + 2]; }
		memcpy(R.box, boxes + 6 * (size_t)i, sizeof R.box);
	}
	return 0;
}

// ---- host: the restatement of the two kernels (test tools; the library runs the kernels) ------------------------------------------
// vertices: the scene's [3 NT][4]; pairs / insts: build_layout's records of the uploaded scene, refit in place.
inline void host_refit(const UpdatePlan &P, const std::vector<InstUpdateRec> &recs, const std::vector<float> &pads, const float *vertices,
                       PairNodeH *pairs, InstH *insts) {
	for (const PaddedBox &b : P.padded) {
		PairNodeH &N = pairs[b.pair];
		float lo[3], hi[3];
		repad_box(b, pads[b.side_mesh >> 1], lo, hi);
		memcpy(b.side_mesh & 1u ? N.lo1 : N.lo0, lo, 12);
		memcpy(b.side_mesh & 1u ? N.hi1 : N.hi0, hi, 12);
	}
	std::vector<UpdateBox> scratch(P.nodes.size());
	for (size_t l = 0; l + 1 < P.level_first.size(); l++)
		for (uint32_t i = P.level_first[l]; i < P.level_first[l + 1]; i++) {
			const UpdateNode &u = P.nodes[i];
			if (u.pair < 0) {
				const uint32_t inst = (uint32_t)u.kid0, m = P.mesh_of_inst[inst];
				const InstUpdateRec &R = recs[inst];
				float lo[3] = {kEmptyLo, kEmptyLo, kEmptyLo}, hi[3] = {kEmptyHi, kEmptyHi, kEmptyHi};
				if (R.valid)
					for (uint32_t q = P.tri_first[m]; q < P.tri_first[m + 1]; q++)
						for (int k = 0; k < 3; k++) {
							float w[3];
							world_point(R.fwd, vertices + 4 * (size_t)(3 * P.tri_list[q] + k), w);
							for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], w[c]); hi[c] = fmaxf(hi[c], w[c]); }
						}
				refit_leaf(R, lo, hi, scratch[i]);
				memcpy(insts[inst].r0, R.r0, 48); // r0, r1, r2
			} else {
				const UpdateBox &a = scratch[u.kid0], &b = scratch[u.kid1];
				float f0, f1;
				refit_inner(a, b, scratch[i], f0, f1);
				PairNodeH &N = pairs[u.pair];
				memcpy(N.lo0, a.blo, 12); memcpy(N.hi0, a.bhi, 12); memcpy(&N.pad0, &f0, 4);
				memcpy(N.lo1, b.blo, 12); memcpy(N.hi1, b.bhi, 12); memcpy(&N.pad1, &f1, 4);
			}
		}
}

#if defined(__HIPCC__)
// ---- device ---------------------------------------------------------------------------------------------------------------------------

// Grid (chunks of a mesh, instances), kExtentBlock threads.  partial: [NI][gridDim.x][6] = lo.xyz, hi.xyz of the chunk's vertices
// (the empty box where the instance's mesh has no triangle in the chunk, or its matrix is singular).  inst_range[i] = first entry
// and number of entries of tri_list for instance i's mesh.  A thread takes every kExtentBlock-th VERTEX of the chunk.
__global__ __launch_bounds__(kExtentBlock) void k_instance_extent(const float4 *__restrict__ vertices, const uint32_t *__restrict__ tri_list,
                                                                   const uint2 *__restrict__ inst_range, const InstUpdateRec *__restrict__ recs,
                                                                   uint32_t num_insts, uint32_t chunk_tris, float *__restrict__ partial) {
	__shared__ float red[kExtentBlock / 64][6];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	for (uint32_t inst = blockIdx.y; inst < num_insts; inst += gridDim.y) {
		const uint2 range = inst_range[inst];
		const InstUpdateRec &R = recs[inst];
		float lo[3] = {kEmptyLo, kEmptyLo, kEmptyLo}, hi[3] = {kEmptyHi, kEmptyHi, kEmptyHi};
		const uint64_t t0 = (uint64_t)blockIdx.x * chunk_tris;
		if (R.valid && t0 < range.y) {
			const uint32_t begin = (uint32_t)t0, end = t0 + chunk_tris < range.y ? (uint32_t)(t0 + chunk_tris) : range.y;
			double fwd[12];
			for (int k = 0; k < 12; k++) fwd[k] = R.fwd[k];
			for (uint64_t v = 3ull * begin + tid; v < 3ull * end; v += kExtentBlock) {
				const uint32_t q = (uint32_t)(v / 3u), k = (uint32_t)(v - 3ull * q);
				const float4 p4 = vertices[3ull * tri_list[range.x + q] + k];
				const float p[3] = {p4.x, p4.y, p4.z};
				float w[3];
				world_point(fwd, p, w);
				for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], w[c]); hi[c] = fmaxf(hi[c], w[c]); }
			}
		}
		for (int c = 0; c < 3; c++)
			for (int off = 32; off > 0; off >>= 1) {
				lo[c] = fminf(lo[c], __shfl_xor(lo[c], off, 64));
				hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off, 64));
			}
		if (lane == 0)
			for (int c = 0; c < 3; c++) { red[wave][c] = lo[c]; red[wave][3 + c] = hi[c]; }
		__syncthreads();
		if (tid < 6) {
			float r = red[0][tid];
			for (uint32_t w = 1; w < kExtentBlock / 64; w++) r = tid < 3 ? fminf(r, red[w][tid]) : fmaxf(r, red[w][tid]);
			partial[((size_t)inst * gridDim.x + blockIdx.x) * 6 + tid] = r;
		}
		__syncthreads(); // (red is written again by the next instance of this workgroup)
	}
}

struct RefitArgs {
	const UpdateNode *nodes;
	const uint32_t *level_first;
	UpdateBox *scratch;             // [plan nodes]
	PairNode *pairs;
	InstRec *insts;
	const InstUpdateRec *recs;
	const float *partial;           // k_instance_extent's
	uint32_t chunks;                // partial boxes per instance
};

__device__ __forceinline__ void store_box(UpdateBox *dst, const UpdateBox &b) { // three 16-byte vector stores
	float4 *d = reinterpret_cast<float4 *>(dst);
	d[0] = make_float4(b.blo[0], b.blo[1], b.blo[2], b.bhi[0]);
	d[1] = make_float4(b.bhi[1], b.bhi[2], b.clo[0], b.clo[1]);
	d[2] = make_float4(b.clo[2], b.chi[0], b.chi[1], b.chi[2]);
}
__device__ __forceinline__ UpdateBox load_box(const UpdateBox *src) {
	const float4 *s = reinterpret_cast<const float4 *>(src);
	const float4 a = s[0], b = s[1], c = s[2];
	return UpdateBox{{a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, c.x}, {c.y, c.z, c.w}};
}

// Levels [level0, level0 + num_levels) of the plan, one thread per node of a level.  More than one level: ONE workgroup, which
// loops over them (a level reads what the level before wrote: workgroup barrier in between); one level: any grid.
__global__ __launch_bounds__(kRefitBlock) void k_refit_top(RefitArgs A, uint32_t level0, uint32_t num_levels) {
	for (uint32_t l = level0; l < level0 + num_levels; l++) {
		const uint32_t end = A.level_first[l + 1];
		for (uint32_t i = A.level_first[l] + blockIdx.x * kRefitBlock + threadIdx.x; i < end; i += gridDim.x * kRefitBlock) {
			const UpdateNode u = A.nodes[i];
			UpdateBox mine;
			if (u.pair < 0) {
				const uint32_t inst = (uint32_t)u.kid0;
				const InstUpdateRec &R = A.recs[inst];
				float lo[3] = {kEmptyLo, kEmptyLo, kEmptyLo}, hi[3] = {kEmptyHi, kEmptyHi, kEmptyHi};
				const float *part = A.partial + (size_t)inst * A.chunks * 6;
				for (uint32_t c = 0; c < A.chunks; c++)
					for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], part[6 * c + k]); hi[k] = fmaxf(hi[k], part[6 * c + 3 + k]); }
				refit_leaf(R, lo, hi, mine);
				InstRec *I = A.insts + inst; // (meta -- root reference and rank -- stays)
				I->r0 = make_float4(R.r0[0], R.r0[1], R.r0[2], R.r0[3]);
				I->r1 = make_float4(R.r1[0], R.r1[1], R.r1[2], R.r1[3]);
				I->r2 = make_float4(R.r2[0], R.r2[1], R.r2[2], R.r2[3]);
			} else {
				const UpdateBox a = load_box(A.scratch + u.kid0), b = load_box(A.scratch + u.kid1);
				float f0, f1;
				refit_inner(a, b, mine, f0, f1);
				PairNode *N = A.pairs + u.pair; // (.w of lo0 / lo1: the child references stay)
				const float ref0 = __int_as_float(reinterpret_cast<const int4 *>(&N->lo0)->w), ref1 = __int_as_float(reinterpret_cast<const int4 *>(&N->lo1)->w);
				N->lo0 = make_float4(a.blo[0], a.blo[1], a.blo[2], ref0);
				N->hi0 = make_float4(a.bhi[0], a.bhi[1], a.bhi[2], f0);
				N->lo1 = make_float4(b.blo[0], b.blo[1], b.blo[2], ref1);
				N->hi1 = make_float4(b.bhi[0], b.bhi[1], b.bhi[2], f1);
			}
			store_box(A.scratch + i, mine);
		}
		if (num_levels > 1) { __threadfence_block(); __syncthreads(); }
	}
}

// One thread per box that leaf subdivision added: the box with the padding a full upload would give it now.  The two sides of a
// pair record are distinct 16-byte words, so two threads never write the same one; .w (reference, cull factor) stays.
__global__ __launch_bounds__(kRefitBlock) void k_repad(const PaddedBox *__restrict__ boxes, uint32_t n, const float *__restrict__ pads, PairNode *pairs) {
	const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
	if (i >= n) return;
	const PaddedBox b = boxes[i];
	float lo[3], hi[3];
	repad_box(b, pads[b.side_mesh >> 1], lo, hi);
	PairNode *N = pairs + b.pair;
	float4 *plo = b.side_mesh & 1u ? &N->lo1 : &N->lo0, *phi = b.side_mesh & 1u ? &N->hi1 : &N->hi0;
	const int4 wlo = *reinterpret_cast<const int4 *>(plo), whi = *reinterpret_cast<const int4 *>(phi);
	*plo = make_float4(lo[0], lo[1], lo[2], __int_as_float(wlo.w));
	*phi = make_float4(hi[0], hi[1], hi[2], __int_as_float(whi.w));
}
#endif // __HIPCC__

} // namespace pol
