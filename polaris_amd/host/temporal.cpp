// temporal.cpp -- the CPU restatement of the temporal reprojection (kernels.h k_reproject, k_reproject_deform, k_temporal), for the
// tests: the same per-pixel arithmetic from polaris_amd/csrc/temporal.h, so the PRIOR, PRIOR2 and TEMPORAL planes of
// polaris_hip_sync_framebuffer are compared with these bit for bit (tests/test_gpu_temporal.py, test_gpu_variance.py,
// test_gpu_motion.py, test_gpu_vertex_motion.py), and their numbers are checked against independent numpy statements of the
// algorithm (tests/test_temporal_cpu.py and its relatives).  The four perspective reprojection entries share their description and argument
// rules with the device's test entries (polaris_amd/csrc/reproject_io.h).
#include <vector>

#include "polaris_hip.h"
#include "reproject_io.h"
#include "temporal.h"

using namespace pol;

namespace {
// THE body of the four reprojection entries below: the PRIOR (M2: and PRIOR2) of every pixel of a checked description, through the
// instantiation of tp_reproject the kernels use for the same groups.  The motion and deformation tables come from the functions the
// library uses (temporal.h, tp_motion_table / tp_deform_table).
template <bool M2, bool MOTION, bool DEFORM>
void reproject_pixels(const ReprojectIo &io) {
	const PolarisTemporalParams &p = *io.p;
	const TpCamera hcam = tp_camera(io.prev_eye, io.prev_frustum), cam = tp_camera(io.eye, io.frustum);
	const uint32_t W = io.W, H = io.H;
	const size_t F = (size_t)W * H;
	const bool ok = tp_projectable(hcam) && p.max_history != 0;
	std::vector<float> table(MOTION ? (size_t)io.n_instances * 16 : 0), dtable(DEFORM ? (size_t)io.n_instances * 16 : 0);
	if (MOTION) tp_motion_table(io.n_instances, io.prev_inv_transforms, io.inv_transforms, table.data());
	if (DEFORM) tp_deform_table(io.n_instances, io.prev_inv_transforms, dtable.data());
	auto load = [&](uint32_t j, TpTap &t) {
		const float *c = io.history + 4 * (size_t)j, *n = io.prev_guide + 4 * (size_t)j;
		t = TpTap{c[0], c[1], c[2], c[3], n[0], n[1], n[2], n[3], io.prev_albedo[4 * (size_t)j + 3],
		          M2 ? io.history_variance[4 * (size_t)j + 1] : 0.0f, MOTION ? io.prev_instance[j] : 0u};
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
				a[3 * k + c] = io.vertices[4 * (3 * (size_t)T + k) + c];
				b[3 * k + c] = io.prev_vertices[4 * (3 * (size_t)T + k) + c];
			}
	};
	for (size_t i = 0; i < F; i++) {
		float *o = io.prior + 4 * i, *o2 = M2 ? io.prior2 + 4 * i : nullptr;
		if (!ok) {
			o[0] = o[1] = o[2] = o[3] = 0.0f;
			if (M2) o2[0] = o2[1] = o2[2] = o2[3] = 0.0f;
			continue;
		}
		tp_reproject<M2, MOTION, DEFORM>((uint32_t)(i % W), (uint32_t)(i / W), W, H, io.guide + 4 * i, io.albedo[4 * i + 3], cam, hcam, p.max_history,
		                                 p.normal_threshold, p.depth_threshold, load, o, o2, MOTION ? io.instance[i] : 0u, io.n_instances, entry_of(table),
		                                 DEFORM ? io.hit + 4 * i : nullptr, io.num_triangles, triangle, entry_of(dtable));
	}
}

// POLARIS_E_BAD_ARGUMENT where reproject_io.h's rules refuse the description, else the instantiation its groups select.
int reproject(const ReprojectIo &io) {
	if (check_reproject(io)) return POLARIS_E_BAD_ARGUMENT;
	const bool m2 = io.m2();
	if (io.deform()) m2 ? reproject_pixels<true, true, true>(io) : reproject_pixels<false, true, true>(io);
	else if (io.motion()) m2 ? reproject_pixels<true, true, false>(io) : reproject_pixels<false, true, false>(io);
	else m2 ? reproject_pixels<true, false, false>(io) : reproject_pixels<false, false, false>(io);
	return POLARIS_OK;
}
} // namespace

extern "C" {

// history (rgb | count), prev_guide, prev_albedo: the history planes under the camera (prev_eye, prev_frustum); guide, albedo: the
// current G-buffer under (eye, frustum); all frame_w * frame_h float4 (row-major).  Writes the PRIOR plane (h rgb | m) of every
// pixel into prior.  POLARIS_E_BAD_ARGUMENT on null pointers, an empty frame or parameters polaris_hip_set_temporal refuses.
int polaris_host_reproject(const float *history, const float *prev_guide, const float *prev_albedo, const float prev_eye[3],
                           const float prev_frustum[16], const float *guide, const float *albedo, const float eye[3], const float frustum[16],
                           uint32_t frame_w, uint32_t frame_h, const PolarisTemporalParams *p, float *prior) {
	return reproject(ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, frame_w, frame_h, p, prior});
}

// PRIOR2 (h2 | 0 | 0 | m) of every pixel: polaris_host_reproject's arguments plus the history's VARIANCE plane hvar.  The PRIOR it
// implies is written to prior (the same bytes as polaris_host_reproject's).
int polaris_host_reproject_moments(const float *history, const float *hvar, const float *prev_guide, const float *prev_albedo, const float prev_eye[3],
                                   const float prev_frustum[16], const float *guide, const float *albedo, const float eye[3], const float frustum[16],
                                   uint32_t frame_w, uint32_t frame_h, const PolarisTemporalParams *p, float *prior, float *prior2) {
	return reproject(ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, frame_w, frame_h, p, prior,
	                             kRpMoments, hvar, prior2});
}

// polaris_host_reproject with object motion (include/polaris_hip.h, polaris_hip_reproject_motion_planes, minus the handle): the two
// INSTANCE planes, the two inv_transform tables of the n_instances mesh instances and, optionally, the history's VARIANCE plane with
// PRIOR2 (both null or neither).
int polaris_host_reproject_motion(const float *history, const float *prev_guide, const float *prev_albedo, const uint32_t *prev_instance,
                                  const float prev_eye[3], const float prev_frustum[16], const float *guide, const float *albedo,
                                  const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t frame_w, uint32_t frame_h,
                                  uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                  const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2) {
	return reproject(ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, frame_w, frame_h, p, prior,
	                             kRpMotion, history_variance, prior2, prev_instance, instance, n_instances, prev_inv_transforms, inv_transforms});
}

// polaris_host_reproject_motion with vertex motion (include/polaris_hip.h, polaris_hip_reproject_deform_planes, minus the handle): the
// current HIT plane (four words per pixel) and the vertices of the num_triangles scene triangles now and as the history saw them.
int polaris_host_reproject_deform(const float *history, const float *prev_guide, const float *prev_albedo, const uint32_t *prev_instance,
                                  const float prev_eye[3], const float prev_frustum[16], const float *guide, const float *albedo,
                                  const uint32_t *instance, const float eye[3], const float frustum[16], uint32_t frame_w, uint32_t frame_h,
                                  uint32_t n_instances, const float *prev_inv_transforms, const float *inv_transforms,
                                  const PolarisTemporalParams *p, const float *history_variance, float *prior, float *prior2,
                                  const uint32_t *hit, const float *vertices, const float *prev_vertices, uint32_t num_triangles) {
	return reproject(ReprojectIo{history, prev_guide, prev_albedo, prev_eye, prev_frustum, guide, albedo, eye, frustum, frame_w, frame_h, p, prior,
	                             kRpDeform, history_variance, prior2, prev_instance, instance, n_instances, prev_inv_transforms, inv_transforms,
	                             hit, vertices, prev_vertices, num_triangles});
}

// ---- polaris_hip_set_projection.  The entries above are untouched and mean kind 0.
namespace {
// The projection as temporal.h takes it; false where polaris_hip_set_projection would not have stored it (the entries below check only
// what they read: the kind and the struct's size).
bool host_projection(const PolarisProjectionParams *proj, TpProjection &P) {
	if (!proj || proj->struct_size != sizeof(PolarisProjectionParams)) return false;
	if (proj->kind != POLARIS_PROJECTION_ORTHOGRAPHIC && proj->kind != POLARIS_PROJECTION_EQUIRECTANGULAR) return false;
	const bool ortho = proj->kind == POLARIS_PROJECTION_ORTHOGRAPHIC;
	P = TpProjection{proj->kind, {proj->axis[0], proj->axis[1], proj->axis[2]}, {proj->right[0], proj->right[1], proj->right[2]},
	                 {proj->up[0], proj->up[1], proj->up[2]}, ortho ? proj->half_width : proj->lon_range, ortho ? proj->half_height : proj->lat_range};
	return true;
}
} // namespace

// polaris_host_reproject under a projection (k_reproject_proj<false, false>): the history camera and the current one share `proj` and
// differ in the eye; there is no frustum.
int polaris_host_reproject_projection(const float *history, const float *prev_guide, const float *prev_albedo, const float prev_eye[3],
                                      const float *guide, const float *albedo, const float eye[3], const PolarisProjectionParams *proj,
                                      uint32_t frame_w, uint32_t frame_h, const PolarisTemporalParams *p, float *prior) {
	TpProjection P;
	if (!history || !prev_guide || !prev_albedo || !prev_eye || !guide || !albedo || !eye || !p || !prior || !host_projection(proj, P)) return POLARIS_E_BAD_ARGUMENT;
	if (frame_w == 0 || frame_h == 0 || p->struct_size != sizeof(PolarisTemporalParams) || tp_check(p->max_history, p->normal_threshold, p->depth_threshold))
		return POLARIS_E_BAD_ARGUMENT;
	const TpProjCamera hcam{P, {prev_eye[0], prev_eye[1], prev_eye[2]}}, cam{P, {eye[0], eye[1], eye[2]}};
	auto load = [&](uint32_t j, TpTap &t) {
		const float *c = history + 4 * (size_t)j, *n = prev_guide + 4 * (size_t)j;
		t = TpTap{c[0], c[1], c[2], c[3], n[0], n[1], n[2], n[3], prev_albedo[4 * (size_t)j + 3], 0.0f, 0u};
	};
	const size_t F = (size_t)frame_w * frame_h;
	for (size_t i = 0; i < F; i++) {
		float *o = prior + 4 * i;
		if (p->max_history == 0) { o[0] = o[1] = o[2] = o[3] = 0.0f; continue; }
		tp_reproject((uint32_t)(i % frame_w), (uint32_t)(i / frame_w), frame_w, frame_h, guide + 4 * i, albedo[4 * i + 3], cam, hcam, p->max_history,
		             p->normal_threshold, p->depth_threshold, load, o);
	}
	return POLARIS_OK;
}

// The guide rays of a projected camera (tp_guide_ray: what k_gbuffer_proj casts): origin and direction of every pixel's centre ray,
// frame_w * frame_h times three floats each.
int polaris_host_projection_rays(const PolarisProjectionParams *proj, const float eye[3], uint32_t frame_w, uint32_t frame_h, float *origins, float *directions) {
	TpProjection P;
	if (!eye || !origins || !directions || frame_w == 0 || frame_h == 0 || !host_projection(proj, P)) return POLARIS_E_BAD_ARGUMENT;
	const TpProjCamera cam{P, {eye[0], eye[1], eye[2]}};
	for (uint32_t gy = 0; gy < frame_h; gy++)
		for (uint32_t gx = 0; gx < frame_w; gx++) {
			const size_t i = (size_t)gy * frame_w + gx;
			tp_guide_ray(cam, gx, gy, 1.0f / (float)frame_w, 1.0f / (float)frame_h, origins + 3 * i, directions + 3 * i);
		}
	return POLARIS_OK;
}

// tp_project of a projected camera for n points (three floats each): uvd = u | v | dist per point, ok = 1 where the projection exists.
int polaris_host_projection_project(const PolarisProjectionParams *proj, const float eye[3], const float *points, uint32_t n, float *uvd, uint8_t *ok) {
	TpProjection P;
	if (!eye || !points || !uvd || !ok || !host_projection(proj, P)) return POLARIS_E_BAD_ARGUMENT;
	const TpProjCamera cam{P, {eye[0], eye[1], eye[2]}};
	for (uint32_t i = 0; i < n; i++) {
		float u = 0.0f, v = 0.0f, dist = 0.0f;
		ok[i] = tp_project(cam, points + 3 * (size_t)i, u, v, dist) ? 1 : 0;
		uvd[3 * (size_t)i] = u; uvd[3 * (size_t)i + 1] = v; uvd[3 * (size_t)i + 2] = dist;
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
