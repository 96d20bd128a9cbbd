// material_update_check.cpp -- CPU harness over polaris_amd/csrc/material_update.h (test tool, not product).
//
// mu_layout: the records build_layout makes of a scene, its tri_bits and emit_classes, and every other array of the layout as one blob.
// mu_update: build_layout of a base scene, then the host restatement of polaris_hip_update_materials (argument checks, the classes of
// the new table, the retag of every triangle record, the mask) applied to it.  tests/test_material_update_cpu.py compares the second
// with the first run on the scene with the materials substituted.
// With -DMU_MAIN: a stand-alone program over a flat file of a base scene and an update, for a sanitizer build (the same comparison).
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -Iinclude -Ipolaris_amd/csrc material_update_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "material_update.h"

using namespace pol;

namespace {

int say(char *err, size_t err_len, const std::string &e) {
	if (err && err_len) { strncpy(err, e.c_str(), err_len - 1); err[err_len - 1] = 0; }
	return 1;
}

std::string layout_of(const PolarisSceneView &sc, int max_leaf_tris, SceneLayout &L) {
	L = SceneLayout();
	std::string e = build_layout(sc, L, max_leaf_tris);
	if (e == "@retry-without-subdivision") { L = SceneLayout(); e = build_layout(sc, L, 0); }
	return e;
}

// Everything of a layout that is neither a triangle record nor derived from materials.
std::vector<uint8_t> rest_of(const SceneLayout &L) {
	std::vector<uint8_t> out;
	auto put = [&](const void *p, size_t n) { out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + n); };
	put(L.pairs.data(), L.pairs.size() * sizeof(PairNodeH));
	put(L.leaves.data(), L.leaves.size() * sizeof(LeafInfoH));
	put(L.insts.data(), L.insts.size() * sizeof(InstH));
	const int32_t misc[4] = {L.root_ref, L.max_stack, (int32_t)L.big_leaves, (int32_t)L.unbounded_boxes};
	put(misc, sizeof misc);
	return out;
}

// The restated update on L, the layout of the uploaded scene `base`.  force_tri_bits: 0, or the tri_bits to pretend the scene has.
int restated_update(const PolarisSceneView &base, SceneLayout &L, const PolarisMaterialUpdate *u, uint32_t force_tri_bits, std::string &msg) {
	const uint32_t tri_bits = force_tri_bits ? force_tri_bits : L.tri_bits;
	const int status = check_material_update(u, true, base.num_material_nodes, base.num_triangles, base.num_emissives, base.num_textures, msg);
	if (status) return status;
	std::vector<uint8_t> cls;
	const uint32_t mask = classify_materials(u->material_nodes, u->num_material_nodes, tri_bits, cls);
	const bool meta = L.tris.size() <= 2046u && base.num_triangles <= 2046u;
	host_retag(L.tris.data(), L.tris.size(), u->material_index ? u->material_index : base.material_index, cls.data(), tri_bits, meta);
	L.emit_classes = mask;
	return 0;
}

} // namespace

extern "C" {

// counts: triangle records, bytes of `rest`; shading: tri_bits, emit_classes
int mu_layout(const PolarisSceneView *sc, int max_leaf_tris, void *tris, void *rest, size_t cap, uint32_t *counts, uint32_t *shading, char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*sc, max_leaf_tris, L);
	if (!e.empty()) return say(err, err_len, e);
	const std::vector<uint8_t> r = rest_of(L);
	if (L.tris.size() * sizeof(TriH) > cap || r.size() > cap) return say(err, err_len, "output buffers too small");
	memcpy(tris, L.tris.data(), L.tris.size() * sizeof(TriH));
	memcpy(rest, r.data(), r.size());
	counts[0] = (uint32_t)L.tris.size(); counts[1] = (uint32_t)r.size();
	shading[0] = L.tri_bits; shading[1] = L.emit_classes;
	return 0;
}

// status: what polaris_hip_update_materials would return (0, or the refusal with its text in err: the records are then build_layout(base)'s).
int mu_update(const PolarisSceneView *base, int max_leaf_tris, const PolarisMaterialUpdate *u, uint32_t force_tri_bits, void *tris, void *rest, size_t cap,
              uint32_t *counts, uint32_t *shading, int *status, char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*base, max_leaf_tris, L);
	if (!e.empty()) return say(err, err_len, e);
	std::string msg;
	*status = restated_update(*base, L, u, force_tri_bits, msg);
	if (*status) say(err, err_len, msg);
	const std::vector<uint8_t> r = rest_of(L);
	if (L.tris.size() * sizeof(TriH) > cap || r.size() > cap) return say(err, err_len, "output buffers too small");
	memcpy(tris, L.tris.data(), L.tris.size() * sizeof(TriH));
	memcpy(rest, r.data(), r.size());
	counts[0] = (uint32_t)L.tris.size(); counts[1] = (uint32_t)r.size();
	shading[0] = L.tri_bits; shading[1] = L.emit_classes;
	return 0;
}

// What polaris_hip_update_texture would return for a scene with the texture metadata `meta`, its text in err.
int mu_texture_check(const PolarisTextureMetadata *meta, uint32_t num_textures, int have_scene, uint32_t index, const void *texels, size_t n_bytes, char *err, size_t err_len) {
	std::string msg;
	const int status = check_texture_update(index, texels, n_bytes, have_scene != 0, std::vector<PolarisTextureMetadata>(meta, meta + num_textures), msg);
	say(err, err_len, msg);
	return status;
}

// The upload's verdict on a scene ("" = accepted): the text an update's refusal must repeat.
int mu_layout_error(const PolarisSceneView *sc, char *err, size_t err_len) {
	SceneLayout L;
	const std::string e = layout_of(*sc, 2, L);
	say(err, err_len, e);
	return e.empty() ? 0 : 1;
}
}

#ifdef MU_MAIN
// File: 15 int64 (the lengths of the ten scene arrays in the order below, scene_diffuse, scene_emissive, then of the update:
// 1 if material_index is given, 1 if emissive nodes are given, the new scene_diffuse); then the arrays: bvh nodes, mesh
// instances, material nodes, emissives, texture metadata, texture data, vertices, normals, uvs, material_index; then the update's:
// material nodes, material_index (if given), emissive nodes (if given).
int main(int argc, char **argv) {
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	int64_t hdr[15];
	if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
	const size_t item[10] = {sizeof(PolarisBvhNode), sizeof(PolarisMeshInstance), sizeof(PolarisMaterialNode), sizeof(PolarisEmissive), sizeof(PolarisTextureMetadata), 1, 16, 16, 8, 4};
	std::vector<std::vector<uint8_t>> a(13);
	auto take = [&](std::vector<uint8_t> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), n, 1, f) == 1; };
	for (int k = 0; k < 10; k++)
		if (!take(a[k], (size_t)hdr[k] * item[k])) return 2;
	if (!take(a[10], a[2].size())) return 2;
	if (hdr[12] && !take(a[11], a[9].size())) return 2;
	if (hdr[13] && !take(a[12], (size_t)hdr[3] * 4)) return 2;
	fclose(f);
	PolarisSceneView base{};
	base.bvh_nodes = (const PolarisBvhNode *)a[0].data(); base.num_bvh_nodes = (uint32_t)hdr[0];
	base.mesh_instances = (const PolarisMeshInstance *)a[1].data(); base.num_mesh_instances = (uint32_t)hdr[1];
	base.material_nodes = (const PolarisMaterialNode *)a[2].data(); base.num_material_nodes = (uint32_t)hdr[2];
	base.emissives = (const PolarisEmissive *)a[3].data(); base.num_emissives = (uint32_t)hdr[3];
	base.texture_meta = (const PolarisTextureMetadata *)a[4].data(); base.num_textures = (uint32_t)hdr[4];
	base.texture_data = a[5].data(); base.texture_data_bytes = (uint32_t)hdr[5];
	base.vertices = (const float *)a[6].data(); base.normals = (const float *)a[7].data(); base.uvs = (const float *)a[8].data();
	base.material_index = (const uint32_t *)a[9].data(); base.num_triangles = (uint32_t)hdr[9];
	base.scene_diffuse_mat_index = (int32_t)hdr[10]; base.scene_emissive_mat_index = (int32_t)hdr[11];
	PolarisMaterialUpdate u{};
	u.struct_size = sizeof u;
	u.material_nodes = (const PolarisMaterialNode *)a[10].data(); u.num_material_nodes = base.num_material_nodes;
	if (hdr[12]) { u.material_index = (const uint32_t *)a[11].data(); u.num_triangles = base.num_triangles; }
	if (hdr[13]) { u.emissive_mat_nodes = (const uint32_t *)a[12].data(); u.num_emissives = base.num_emissives; }
	u.scene_diffuse_mat_index = (int32_t)hdr[14];
	// the substituted scene
	std::vector<PolarisEmissive> ems(base.emissives, base.emissives + base.num_emissives);
	for (uint32_t e = 0; hdr[13] && e < base.num_emissives; e++) ems[e].mat_node_index = u.emissive_mat_nodes[e];
	PolarisSceneView sub = base;
	sub.material_nodes = u.material_nodes;
	if (u.material_index) sub.material_index = u.material_index;
	sub.emissives = ems.data();
	sub.scene_diffuse_mat_index = u.scene_diffuse_mat_index;
	for (int max_leaf : {0, 2, 4}) {
		SceneLayout A, B;
		std::string e = layout_of(base, max_leaf, A), msg;
		if (e.empty()) e = layout_of(sub, max_leaf, B);
		if (!e.empty()) { fprintf(stderr, "layout: %s\n", e.c_str()); return 1; }
		if (restated_update(base, A, &u, 0, msg)) { fprintf(stderr, "refused: %s\n", msg.c_str()); return 1; }
		if (A.tris.size() != B.tris.size() || memcmp(A.tris.data(), B.tris.data(), A.tris.size() * sizeof(TriH)) || A.emit_classes != B.emit_classes || A.tri_bits != B.tri_bits ||
		    rest_of(A) != rest_of(B)) {
			fprintf(stderr, "max_leaf_tris %d: the restated update differs from the layout of the substituted scene\n", max_leaf);
			return 1;
		}
		SceneLayout C31;
		layout_of(base, max_leaf, C31);
		const std::vector<TriH> before = C31.tris;
		if (restated_update(base, C31, &u, 31, msg) || memcmp(before.data(), C31.tris.data(), before.size() * sizeof(TriH)) || C31.emit_classes != 0xFFFFu) {
			fprintf(stderr, "tri_bits 31: records or mask changed\n");
			return 1;
		}
	}
	printf("ok\n");
	return 0;
}
#endif
