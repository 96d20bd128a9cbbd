// temporal.cpp -- the CPU restatement of the temporal reprojection (kernels.h k_reproject, k_temporal), for the tests: the same
// per-pixel arithmetic from polaris_amd/csrc/temporal.h, so the PRIOR and TEMPORAL planes of polaris_hip_sync_framebuffer are
// compared with these bit for bit (tests/test_gpu_temporal.py), and their numbers are checked against an independent numpy
// statement of the algorithm (tests/test_temporal_cpu.py).
#include <vector>

#include "polaris_hip.h"
#include "temporal.h"

using namespace pol;

extern "C" {

// history (rgb | count), prev_guide, prev_albedo: the history planes under the camera (prev_eye, prev_frustum); guide, albedo: the
// current G-buffer under (eye, frustum); all frame_w * frame_h float4 (row-major).  Writes the PRIOR plane (h rgb | m) of every
// pixel into prior.  POLARIS_E_BAD_ARGUMENT on null pointers, an empty frame or parameters polaris_hip_set_temporal refuses.
int polaris_host_reproject(const float *history, const float *prev_guide, const float *prev_albedo, const float prev_eye[3],
                           const float prev_frustum[16], const float *guide, const float *albedo, const float eye[3], const float frustum[16],
                           uint32_t frame_w, uint32_t frame_h, const PolarisTemporalParams *p, float *prior) {
	if (!history || !prev_guide || !prev_albedo || !prev_eye || !prev_frustum || !guide || !albedo || !eye || !frustum || !p || !prior)
		return POLARIS_E_BAD_ARGUMENT;
	if (p->struct_size != sizeof(PolarisTemporalParams)) return POLARIS_E_BAD_ARGUMENT;
	if (tp_check(p->max_history, p->normal_threshold, p->depth_threshold)) return POLARIS_E_BAD_ARGUMENT;
	if (frame_w == 0 || frame_h == 0 || (uint64_t)frame_w * frame_h > (1ull << 26)) return POLARIS_E_BAD_ARGUMENT;
	auto camera = [](const float e[3], const float f[16]) {
		return TpCamera{{f[0], f[1], f[2], f[3]}, {f[4], f[5], f[6], f[7]}, {f[8], f[9], f[10], f[11]}, {f[12], f[13], f[14], f[15]}, {e[0], e[1], e[2]}};
	};
	const TpCamera hcam = camera(prev_eye, prev_frustum), cam = camera(eye, frustum);
	const uint32_t W = frame_w, H = frame_h;
	const size_t F = (size_t)W * H;
	const bool ok = tp_projectable(hcam) && p->max_history != 0;
	auto load = [&](uint32_t j, TpTap &t) {
		const float *c = history + 4 * (size_t)j, *n = prev_guide + 4 * (size_t)j;
		t = TpTap{c[0], c[1], c[2], c[3], n[0], n[1], n[2], n[3], prev_albedo[4 * (size_t)j + 3], 0.0f, 0u};
	};
	for (size_t i = 0; i < F; i++) {
		float *o = prior + 4 * i;
		if (!ok) {
			o[0] = o[1] = o[2] = o[3] = 0.0f;
			continue;
		}
		tp_reproject((uint32_t)(i % W), (uint32_t)(i / W), W, H, guide + 4 * i, albedo[4 * i + 3], cam, hcam, p->max_history, p->normal_threshold,
		             p->depth_threshold, load, o);
	}
	return POLARIS_OK;
}

// polaris_host_reproject with object motion (include/polaris_hip.h, polaris_hip_reproject_motion_planes, minus the handle): the two
// INSTANCE planes, the two inv_transform tables of the n_instances mesh instances and, optionally, the history's VARIANCE plane with
// PRIOR2 (both null or neither).  The motion table comes from the function the library uses (temporal.h, tp_motion_table).
int polaris_host_reproject_motion(const float *history, const float *prev_guide, const float *prev_albedo, const uint32_t *prev_instance,
                                  const float prev_eye[3], const float prev_frustum[16], const float *guide, const float *albedo,
                                  const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t frame_w, uint32_t frame_h,
                                  uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                  const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2) {
	if (!history || !prev_guide || !prev_albedo || !prev_instance || !prev_eye || !prev_frustum || !guide || !albedo || !instance || !eye ||
	    !frustum || !prev_inv_transforms || !inv_transforms || !p || !prior)
		return POLARIS_E_BAD_ARGUMENT;
	if ((history_variance == nullptr) != (prior2 == nullptr)) return POLARIS_E_BAD_ARGUMENT;
	if (p->struct_size != sizeof(PolarisTemporalParams)) return POLARIS_E_BAD_ARGUMENT;
	if (tp_check(p->max_history, p->normal_threshold, p->depth_threshold)) return POLARIS_E_BAD_ARGUMENT;
	if (frame_w == 0 || frame_h == 0 || (uint64_t)frame_w * frame_h > (1ull << 26)) return POLARIS_E_BAD_ARGUMENT;
	if (n_instances == 0 || n_instances > kTpMaxInstances) return POLARIS_E_BAD_ARGUMENT;
	auto camera = [](const float e[3], const float f[16]) {
		return TpCamera{{f[0], f[1], f[2], f[3]}, {f[4], f[5], f[6], f[7]}, {f[8], f[9], f[10], f[11]}, {f[12], f[13], f[14], f[15]}, {e[0], e[1], e[2]}};
	};
	const TpCamera hcam = camera(prev_eye, prev_frustum), cam = camera(eye, frustum);
	const uint32_t W = frame_w, H = frame_h;
	const size_t F = (size_t)W * H;
	const bool ok = tp_projectable(hcam) && p->max_history != 0;
	std::vector<float> table((size_t)n_instances * 16);
	tp_motion_table(n_instances, prev_inv_transforms, inv_transforms, table.data());
	auto load = [&](uint32_t j, TpTap &t) {
		const float *c = history + 4 * (size_t)j, *n = prev_guide + 4 * (size_t)j;
		t = TpTap{c[0], c[1], c[2], c[3], n[0], n[1], n[2], n[3], prev_albedo[4 * (size_t)j + 3],
		          history_variance ? history_variance[4 * (size_t)j + 1] : 0.0f, prev_instance[j]};
	};
	auto entry = [&](uint32_t k, float *D) -> uint32_t {
		const float *e = table.data() + 16 * (size_t)k;
		for (int c = 0; c < 12; c++) D[c] = e[c];
		return pm_f2u(e[12]);
	};
	for (size_t i = 0; i < F; i++) {
		float *o = prior + 4 * i, *o2 = prior2 ? prior2 + 4 * i : nullptr;
		if (!ok) {
			o[0] = o[1] = o[2] = o[3] = 0.0f;
			if (o2) o2[0] = o2[1] = o2[2] = o2[3] = 0.0f;
			continue;
		}
		const uint32_t gx = (uint32_t)(i % W), gy = (uint32_t)(i / W);
		if (o2)
			tp_reproject<true, true>(gx, gy, W, H, guide + 4 * i, albedo[4 * i + 3], cam, hcam, p->max_history, p->normal_threshold, p->depth_threshold,
			                         load, o, o2, instance[i], n_instances, entry);
		else
			tp_reproject<false, true>(gx, gy, W, H, guide + 4 * i, albedo[4 * i + 3], cam, hcam, p->max_history, p->normal_threshold, p->depth_threshold,
			                          load, o, nullptr, instance[i], n_instances, entry);
	}
	return POLARIS_OK;
}

// polaris_host_reproject_motion with vertex motion (include/polaris_hip.h, polaris_hip_reproject_deform_planes, minus the handle): the
// current HIT plane (four words per pixel) and the vertices of the num_triangles scene triangles now and as the history saw them.
int polaris_host_reproject_deform(const float *history, const float *prev_guide, const float *prev_albedo, const uint32_t *prev_instance,
                                  const float prev_eye[3], const float prev_frustum[16], const float *guide, const float *albedo,
                                  const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t frame_w, uint32_t frame_h,
                                  uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                  const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2,
                                  const uint32_t *hit, const float *vertices, const float *prev_vertices, uint32_t num_triangles) {
	if (!history || !prev_guide || !prev_albedo || !prev_instance || !prev_eye || !prev_frustum || !guide || !albedo || !instance || !eye ||
	    !frustum || !prev_inv_transforms || !inv_transforms || !p || !prior || !hit || !vertices || !prev_vertices)
		return POLARIS_E_BAD_ARGUMENT;
	if ((history_variance == nullptr) != (prior2 == nullptr)) return POLARIS_E_BAD_ARGUMENT;
	if (p->struct_size != sizeof(PolarisTemporalParams)) return POLARIS_E_BAD_ARGUMENT;
	if (tp_check(p->max_history, p->normal_threshold, p->depth_threshold)) return POLARIS_E_BAD_ARGUMENT;
	if (frame_w == 0 || frame_h == 0 || (uint64_t)frame_w * frame_h > (1ull << 26)) return POLARIS_E_BAD_ARGUMENT;
	if (n_instances == 0 || n_instances > kTpMaxInstances || num_triangles == 0 || num_triangles > kTpMaxTriangles) return POLARIS_E_BAD_ARGUMENT;
	auto camera = [](const float e[3], const float f[16]) {
		return TpCamera{{f[0], f[1], f[2], f[3]}, {f[4], f[5], f[6], f[7]}, {f[8], f[9], f[10], f[11]}, {f[12], f[13], f[14], f[15]}, {e[0], e[1], e[2]}};
	};
	const TpCamera hcam = camera(prev_eye, prev_frustum), cam = camera(eye, frustum);
	const uint32_t W = frame_w, H = frame_h;
	const size_t F = (size_t)W * H;
	const bool ok = tp_projectable(hcam) && p->max_history != 0;
	std::vector<float> table((size_t)n_instances * 16), dtable((size_t)n_instances * 16);
	tp_motion_table(n_instances, prev_inv_transforms, inv_transforms, table.data());
	tp_deform_table(n_instances, prev_inv_transforms, dtable.data());
	auto load = [&](uint32_t j, TpTap &t) {
		const float *c = history + 4 * (size_t)j, *n = prev_guide + 4 * (size_t)j;
		t = TpTap{c[0], c[1], c[2], c[3], n[0], n[1], n[2], n[3], prev_albedo[4 * (size_t)j + 3],
		          history_variance ? history_variance[4 * (size_t)j + 1] : 0.0f, prev_instance[j]};
	};
	auto entry_of = [](const std::vector<float> &tab) {
		return [&tab](uint32_t k, float *D) -> uint32_t {
			const float *e = tab.data() + 16 * (size_t)k;
			for (int c = 0; c < 12; c++) D[c] = e[c];
			return pm_f2u(e[12]);
		};
	};
	auto triangle = [&](uint32_t T, float *a, float *b) {
		for (int k = 0; k < 3; k++)
			for (int c = 0; c < 3; c++) {
				a[3 * k + c] = vertices[4 * (3 * (size_t)T + k) + c];
				b[3 * k + c] = prev_vertices[4 * (3 * (size_t)T + k) + c];
			}
	};
	for (size_t i = 0; i < F; i++) {
		float *o = prior + 4 * i, *o2 = prior2 ? prior2 + 4 * i : nullptr;
		if (!ok) {
			o[0] = o[1] = o[2] = o[3] = 0.0f;
			if (o2) o2[0] = o2[1] = o2[2] = o2[3] = 0.0f;
			continue;
		}
		const uint32_t gx = (uint32_t)(i % W), gy = (uint32_t)(i / W);
		if (o2)
			tp_reproject<true, true, true>(gx, gy, W, H, guide + 4 * i, albedo[4 * i + 3], cam, hcam, p->max_history, p->normal_threshold, p->depth_threshold,
			                               load, o, o2, instance[i], n_instances, entry_of(table), hit + 4 * i, num_triangles, triangle, entry_of(dtable));
		else
			tp_reproject<false, true, true>(gx, gy, W, H, guide + 4 * i, albedo[4 * i + 3], cam, hcam, p->max_history, p->normal_threshold, p->depth_threshold,
			                                load, o, nullptr, instance[i], n_instances, entry_of(table), hit + 4 * i, num_triangles, triangle, entry_of(dtable));
	}
	return POLARIS_OK;
}

// tp_motion_matrix for the tests: the flag (0 STATIC, 1 MOVED, 2 INVALID) and D's twelve floats (rows r0, r1, r2).
int polaris_host_motion_matrix(const float inv_hist[16], const float inv_cur[16], uint32_t *flag, float D[12]) {
	if (!inv_hist || !inv_cur || !flag || !D) return POLARIS_E_BAD_ARGUMENT;
	*flag = tp_motion_matrix(inv_hist, inv_cur, D);
	return POLARIS_OK;
}

// The TEMPORAL rows [block_y, block_y + block_h) from frame_acc and prior (frame_w * frame_h float4) into out; its other rows are not
// written.  n = accumulated_samples + samples_per_pixel; the weight is sync's (float)(1.0 / (float)n).
int polaris_host_temporal_combine(const float *frame_acc, const float *prior, uint32_t accumulated_samples, uint32_t samples_per_pixel,
                                  uint32_t frame_w, uint32_t frame_h, uint32_t block_y, uint32_t block_h, float *out) {
	if (!frame_acc || !prior || !out) return POLARIS_E_BAD_ARGUMENT;
	if (frame_w == 0 || frame_h == 0 || block_h == 0 || (uint64_t)block_y + block_h > frame_h) return POLARIS_E_BAD_ARGUMENT;
	if (accumulated_samples + samples_per_pixel == 0) return POLARIS_E_BAD_ARGUMENT;
	const float n = (float)(accumulated_samples + samples_per_pixel);
	const float weight = (float)(1.0 / (float)(accumulated_samples + samples_per_pixel)); // (polaris_hip_sync_framebuffer's)
	for (size_t i = (size_t)block_y * frame_w; i < (size_t)(block_y + block_h) * frame_w; i++)
		tp_combine(frame_acc + 4 * i, prior + 4 * i, n, weight, out + 4 * i);
	return POLARIS_OK;
}

} // extern "C"
