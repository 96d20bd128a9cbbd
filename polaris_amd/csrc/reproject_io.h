// reproject_io.h -- ONE description of a reprojection of caller planes and ONE set of argument rules for it, shared by the device
// test entries (polaris_hip.hip: polaris_hip_reproject_planes, _reproject_motion_planes, _reproject_deform_planes) and their CPU
// restatements (polaris_amd/host/temporal.cpp: polaris_host_reproject, _reproject_moments, _reproject_motion, _reproject_deform),
// which the bit-for-bit tests compare with each other: the two sides cannot disagree about what they refuse.  The frame and row
// rules of every *_planes entry live here too.  Host only, plain C++: no device code, no HIP.
#pragma once

#include <stdint.h>

#include "polaris_hip.h"
#include "temporal.h"

namespace pol {

// The rules, one text each (plane_rule_text).  0: the arguments are valid.
enum PlaneRule : int {
	kRuleOk = 0,
	kRuleNull,         // a pointer of the required group
	kRuleStructSize,
	kRuleParams,       // tp_check
	kRuleFrame,
	kRuleRows,
	kRuleMomentsPair,  // one of history_variance / prior2 without the other
	kRuleMomentsNull,  // an entry that requires the moments group
	kRuleMotionNull,
	kRuleInstances,
	kRuleDeformNull,
	kRuleTriangles,
	kRuleCount
};
static_assert(kTpMaxHistory == 4096 && kTpMaxDepthThreshold == 1e6f && kTpMaxInstances == 1u << 20 && kTpMaxTriangles == 1u << 24, "the texts below state these limits");
inline const char *plane_rule_text(int rule) {
	static const char *const text[kRuleCount] = {
		"ok",
		"null plane, camera, params or prior pointer",
		"params: struct_size is not sizeof(PolarisTemporalParams)",
		"params: max_history 0..4096, normal_threshold [-1, 1], depth_threshold [0, 1e6]",
		"frame of 1..2^26 pixels",
		"rows [block_y, +block_h): at least one, inside the frame",
		"history_variance without prior2 (or the reverse)",
		"null history_variance or prior2",
		"null INSTANCE plane or inv_transform table",
		"1..2^20 instances",
		"null HIT plane or vertices",
		"1..2^24 triangles",
	};
	return rule >= 0 && rule < kRuleCount ? text[rule] : "?";
}

constexpr uint64_t kPlaneMaxPixels = 1ull << 26; // of every *_planes entry and of the four restatements
inline int check_frame(uint32_t W, uint32_t H) { return W == 0 || H == 0 || (uint64_t)W * H > kPlaneMaxPixels ? kRuleFrame : kRuleOk; }
inline int check_rows(uint32_t H, uint32_t block_y, uint32_t block_h) { return block_h == 0 || (uint64_t)block_y + block_h > H ? kRuleRows : kRuleOk; }

// The groups of a ReprojectIo beyond the required one (DEFORM extends MOTION, as tp_reproject's template parameters).
enum : uint32_t { kRpMoments = 1u, kRpMotion = 2u, kRpDeform = 4u | kRpMotion };

// One reprojection of caller planes (frame-sized, row major; float4 planes unless noted).  An entry fills the groups it has
// arguments for and names in `need` the ones it demands; the others stay null / 0.
struct ReprojectIo {
	// required: the history under (prev_eye, prev_frustum), the current G-buffer under (eye, frustum), the PRIOR written
	const float *history, *prev_guide, *prev_albedo, *prev_eye, *prev_frustum, *guide, *albedo, *eye, *frustum;
	uint32_t W, H;
	const PolarisTemporalParams *p;
	float *prior;
	uint32_t need = 0;
	// moments: the history's VARIANCE plane and PRIOR2 -- both or neither; both where need has kRpMoments
	const float *history_variance = nullptr;
	float *prior2 = nullptr;
	// motion (need has kRpMotion): the two INSTANCE planes (one word a pixel) and the two inv_transform tables of the n_instances instances
	const uint32_t *prev_instance = nullptr, *instance = nullptr;
	uint32_t n_instances = 0;
	const float *prev_inv_transforms = nullptr, *inv_transforms = nullptr;
	// deform (need has kRpDeform, which has kRpMotion): the current HIT plane (four words a pixel), the vertices now and as the history saw them
	const uint32_t *hit = nullptr;
	const float *vertices = nullptr, *prev_vertices = nullptr;
	uint32_t num_triangles = 0;

	bool m2() const { return prior2 != nullptr; } // (after check_reproject: history_variance is there too)
	bool motion() const { return (need & kRpMotion) != 0; }
	bool deform() const { return (need & kRpDeform) == kRpDeform; }
};

// The one place that knows the limits of a reprojection's arguments.  Nothing behind a caller's pointer is read but *p.
inline int check_reproject(const ReprojectIo &io) {
	if (!io.history || !io.prev_guide || !io.prev_albedo || !io.prev_eye || !io.prev_frustum || !io.guide || !io.albedo || !io.eye || !io.frustum ||
	    !io.p || !io.prior)
		return kRuleNull;
	if (io.p->struct_size != sizeof(PolarisTemporalParams)) return kRuleStructSize;
	if (tp_check(io.p->max_history, io.p->normal_threshold, io.p->depth_threshold)) return kRuleParams;
	if (const int rule = check_frame(io.W, io.H)) return rule;
	if ((io.history_variance == nullptr) != (io.prior2 == nullptr)) return kRuleMomentsPair;
	if ((io.need & kRpMoments) && !io.prior2) return kRuleMomentsNull;
	if (io.motion()) {
		if (!io.prev_instance || !io.instance || !io.prev_inv_transforms || !io.inv_transforms) return kRuleMotionNull;
		if (io.n_instances == 0 || io.n_instances > kTpMaxInstances) return kRuleInstances;
	}
	if (io.deform()) {
		if (!io.hit || !io.vertices || !io.prev_vertices) return kRuleDeformNull;
		if (io.num_triangles == 0 || io.num_triangles > kTpMaxTriangles) return kRuleTriangles;
	}
	return kRuleOk;
}

} // namespace pol
