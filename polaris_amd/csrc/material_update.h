// material_update.h -- editing materials in place: polaris_hip_update_materials / polaris_hip_update_texture.
//
// When only materials change, geometry, trees, slot order, node mode and the kernel variants of the uploaded scene stay; what changes
// is the node table, the triangles' roots, the background node, the emissives' material nodes -- plain copies -- and the two things an
// upload DERIVES from the node table and keeps elsewhere:
//
//   the shading class of every triangle   node_class[material_index[t]] (scene_layout.h shading_classes), packed into two words of the
//                                         slot's 48-byte record: orig = triangle | class << tri_bits, and for scenes of at most 2 046
//                                         slots pad2 = tiny_meta_word(rank, orig).  The traversal kernels hand it to the hit record.
//   SceneT::emit_classes                  the classes that can end in an emitter (emitting_classes): the shade prefilter reads a clear
//                                         bit as a promise (kernels.h shade_fate), so a stale one loses radiance.
//
// The host classifies the NEW table, O(nodes); the device retags every record:
//
//   k_retag  one thread per triangle slot (kRetagSlotsPerThread of them, a workgroup apart): t = orig & mask, c = cls[mat_index[t]],
//            orig = t | c << tri_bits, pad2 = tiny_meta_word(rank, orig) where the scene carries it.  The 16-byte words that hold orig
//            and pad2 are read and written whole; v0 | rank is never written.  No two threads touch the same record.  The class table
//            (a byte per node) is staged in LDS when it has at most kRetagLdsNodes entries.
//
// tri_bits == 31 (more than 2^24 triangles): hits carry no class, nothing is retagged and emit_classes stays all ones.
//
// The per-slot arithmetic (retag_slot) is __host__ __device__: host_retag below is the same code on the CPU, and
// tests/tools/material_update_check.cpp shows it byte-equal to build_layout of the scene with the new materials.
#pragma once

#include "polaris_hip.h"
#include "scene_layout.h"
#if defined(__HIPCC__)
#include "kernels.h"
#endif

namespace pol {

constexpr uint32_t kRetagBlock = 256;
constexpr uint32_t kRetagSlotsPerThread = 4;  // a workgroup retags kRetagBlock * kRetagSlotsPerThread slots: one staging of the table for all of them
constexpr uint32_t kRetagLdsNodes = 1024;     // class tables up to this many nodes are staged in LDS: at most a dword per thread

// The words of one triangle slot after the edit.  rank / orig / pad2: the record's three .w words (pad2 and rank are only used with
// `meta`: the scene's slots carry the tiny meta word).  cls: the class of every node of the NEW table, in whatever address space.
template <class ClassTable>
POL_HD inline void retag_slot(uint32_t rank, uint32_t &orig, uint32_t &pad2, const uint32_t *mat_index, ClassTable cls, uint32_t tri_bits, bool meta) {
	const uint32_t t = orig & ((1u << tri_bits) - 1u);
	orig = t | (uint32_t)cls[mat_index[t]] << tri_bits;
	if (meta) pad2 = tiny_meta_word(rank, orig);
}

// Bytes of a texture's texels: build_layout's expression.
inline uint64_t texture_bytes(const PolarisTextureMetadata &m) {
	const uint64_t bpp = m.format == POLARIS_TEX_L8 ? 1 : (m.format == POLARIS_TEX_RGBA32F ? 16 : 4);
	return bpp * m.width * m.height;
}

// ---- host: the argument checks of polaris_hip_update_materials, none of which needs the device -------------------------------------------
// num_nodes, NT, num_emissives, num_textures: the uploaded scene's counts.  0 = accepted, else the POLARIS_E_* status the entry returns,
// with msg.  The material rules are the upload's (scene_layout.h check_materials), with its texts.
inline int check_material_update(const PolarisMaterialUpdate *u, bool have_scene, uint32_t num_nodes, uint32_t NT, uint32_t num_emissives, uint32_t num_textures,
                                 std::string &msg) {
	if (!u) { msg = "material update is null"; return POLARIS_E_BAD_ARGUMENT; }
	if (!have_scene) { msg = "no scene data uploaded"; return POLARIS_E_NO_SCENE_DATA; }
	if (u->struct_size != sizeof(PolarisMaterialUpdate)) { msg = "update_materials: struct_size is not sizeof(PolarisMaterialUpdate)"; return POLARIS_E_BAD_ARGUMENT; }
	if (!u->material_nodes) { msg = "update_materials: material node pointer is null"; return POLARIS_E_BAD_ARGUMENT; }
	if (u->num_material_nodes != num_nodes) {
		msg = "update_materials: " + std::to_string(u->num_material_nodes) + " material nodes, the uploaded scene has " + std::to_string(num_nodes);
		return POLARIS_E_BAD_ARGUMENT;
	}
	if (u->material_index && u->num_triangles != NT) {
		msg = "update_materials: " + std::to_string(u->num_triangles) + " triangles, the uploaded scene has " + std::to_string(NT);
		return POLARIS_E_BAD_ARGUMENT;
	}
	if (u->emissive_mat_nodes && u->num_emissives != num_emissives) {
		msg = "update_materials: " + std::to_string(u->num_emissives) + " emissives, the uploaded scene has " + std::to_string(num_emissives);
		return POLARIS_E_BAD_ARGUMENT;
	}
	PolarisSceneView v{};
	v.material_nodes = u->material_nodes; v.num_material_nodes = num_nodes;
	v.num_textures = num_textures;
	v.material_index = u->material_index; v.num_triangles = NT;
	v.num_emissives = u->emissive_mat_nodes ? num_emissives : 0;
	v.scene_diffuse_mat_index = u->scene_diffuse_mat_index;
	msg = check_materials(v, u->emissive_mat_nodes);
	return msg.empty() ? 0 : POLARIS_E_BAD_SCENE;
}

// ... and of polaris_hip_update_texture.  meta: the uploaded scene's texture metadata.
inline int check_texture_update(uint32_t index, const void *texels, size_t n_bytes, bool have_scene, const std::vector<PolarisTextureMetadata> &meta, std::string &msg) {
	if (!have_scene) { msg = "no scene data uploaded"; return POLARIS_E_NO_SCENE_DATA; }
	if (index >= meta.size()) {
		msg = "update_texture: texture " + std::to_string(index) + " out of range, the uploaded scene has " + std::to_string(meta.size());
		return POLARIS_E_BAD_ARGUMENT;
	}
	if (!texels) { msg = "update_texture: texel pointer is null"; return POLARIS_E_BAD_ARGUMENT; }
	if ((uint64_t)n_bytes != texture_bytes(meta[index])) {
		msg = "update_texture: " + std::to_string(n_bytes) + " bytes, texture " + std::to_string(index) + " has " + std::to_string(texture_bytes(meta[index]));
		return POLARIS_E_BAD_ARGUMENT;
	}
	return 0;
}

// ---- host: what an upload derives from the node table -----------------------------------------------------------------------------
// cls: the class of every node (padded with zeros to whole dwords: the device stages it by the dword); the return value: emit_classes.
inline uint32_t classify_materials(const PolarisMaterialNode *nodes, uint32_t num_nodes, uint32_t tri_bits, std::vector<uint8_t> &cls) {
	PolarisSceneView v{};
	v.material_nodes = nodes; v.num_material_nodes = num_nodes;
	shading_classes(v, cls);
	const uint32_t mask = tri_bits < 31 ? emitting_classes(v, cls) : 0xFFFFu;
	cls.resize(((size_t)num_nodes + 3) / 4 * 4, 0);
	return mask;
}

// ---- host: the restatement of k_retag (test tools; the library runs the kernel) ----------------------------------------------------
// tris: build_layout's records of the uploaded scene, retagged in place; mat_index: the scene's roots after the edit; meta: the slots
// carry the tiny meta word (build_layout: at most 2 046 slots and triangles).
inline void host_retag(TriH *tris, size_t num_slots, const uint32_t *mat_index, const uint8_t *cls, uint32_t tri_bits, bool meta) {
	if (tri_bits >= 31) return;
	for (size_t s = 0; s < num_slots; s++) retag_slot(tris[s].rank, tris[s].orig, tris[s].pad2, mat_index, cls, tri_bits, meta);
}

#if defined(__HIPCC__)
// ---- device ---------------------------------------------------------------------------------------------------------------------------

// cls: [num_nodes] bytes in whole dwords.  tri_bits < 31 (the host launches nothing otherwise).  The second and third 16-byte word of a
// record are read and written whole (the third only with `meta`); the first is only read for the rank.
__global__ __launch_bounds__(kRetagBlock) void k_retag(TriRec *tris, uint32_t num_slots, const uint32_t *__restrict__ mat_index, const uint8_t *__restrict__ cls,
                                                       uint32_t num_nodes, uint32_t tri_bits, uint32_t meta) {
	__shared__ uint32_t lcls[kRetagLdsNodes / 4];
	const bool staged = num_nodes <= kRetagLdsNodes; // (uniform)
	if (staged) {
		for (uint32_t w = threadIdx.x; 4 * w < num_nodes; w += kRetagBlock) lcls[w] = reinterpret_cast<const uint32_t *>(cls)[w];
		__syncthreads();
	}
	const uint32_t first = blockIdx.x * (kRetagBlock * kRetagSlotsPerThread) + threadIdx.x;
	for (uint32_t k = 0; k < kRetagSlotsPerThread; k++) {
		const uint32_t s = first + k * kRetagBlock;
		if (s >= num_slots) break;
		uint4 *rec = reinterpret_cast<uint4 *>(tris + s);
		uint4 e1 = rec[1], e2 = make_uint4(0, 0, 0, 0);
		uint32_t rank = 0;
		if (meta) { e2 = rec[2]; rank = reinterpret_cast<const uint32_t *>(rec)[3]; }
		if (staged) retag_slot(rank, e1.w, e2.w, mat_index, reinterpret_cast<const uint8_t *>(lcls), tri_bits, meta != 0);
		else retag_slot(rank, e1.w, e2.w, mat_index, cls, tri_bits, meta != 0);
		rec[1] = e1;
		if (meta) rec[2] = e2;
	}
}

// The material node of every emissive record: one thread per entry, nothing else of the record changes.
__global__ __launch_bounds__(kRetagBlock) void k_emissive_nodes(PolarisEmissive *emissives, const uint32_t *__restrict__ nodes, uint32_t n) {
	const uint32_t e = blockIdx.x * kRetagBlock + threadIdx.x;
	if (e < n) emissives[e].mat_node_index = nodes[e];
}
#endif // __HIPCC__

} // namespace pol
