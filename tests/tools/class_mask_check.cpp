// class_mask_check.cpp -- test tap for scene_layout.h's shading classes and the mask of classes that can end in an emitter
// (tests/test_class_mask.py): the two functions on a caller-supplied material node table, nothing else of a scene.
#include "scene_layout.h"

extern "C" int class_mask_check(const PolarisMaterialNode *nodes, uint32_t n, uint8_t *cls_out, uint32_t *mask_out) {
	PolarisSceneView sc{};
	sc.material_nodes = nodes;
	sc.num_material_nodes = n;
	std::vector<uint8_t> cls;
	pol::shading_classes(sc, cls);
	for (uint32_t i = 0; i < n; i++) cls_out[i] = cls[i];
	*mask_out = pol::emitting_classes(sc, cls);
	return 0;
}
