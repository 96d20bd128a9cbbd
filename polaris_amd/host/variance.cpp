// variance.cpp -- the CPU restatement of variance guidance (kernels.h k_variance, k_denoise_variance), for the
// tests: the same per-pixel arithmetic from polaris_amd/csrc/variance.h, the same iteration order, so the VARIANCE and
// DENOISED planes of polaris_hip_sync_framebuffer are compared with these bit for bit (tests/test_gpu_variance.py), and their
// numbers are checked against an independent numpy statement of the algorithm (tests/test_variance_cpu.py).
#include <vector>

#include "polaris_hip.h"
#include "variance.h"

using namespace pol;

namespace {
bool rows_ok(uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h) {
	return W != 0 && H != 0 && block_h != 0 && (uint64_t)block_y + block_h <= H;
}
bool params_ok(const PolarisDenoiseParams *p, const PolarisVarianceParams *v) {
	return p && v && p->struct_size == sizeof(PolarisDenoiseParams) && v->struct_size == sizeof(PolarisVarianceParams) &&
	       !dn_check(p->iterations, p->normal_power_log2, p->sigma_depth, p->sigma_luminance) && v->sigma_variance != 0.0f &&
	       !va_check(v->sigma_variance, v->min_samples);
}
} // namespace

extern "C" {

// The VARIANCE rows [block_y, block_y + block_h) into out (frame_w * frame_h float4; its other rows are not written).  frame_acc: rgb |
// sum L^2 of `samples` = accumulated_samples + samples_per_pixel samples; temporal (TEMPORAL plane) and prior2 (h2 | 0 | 0 | m) are
// both null without temporal reuse, else both given.  POLARIS_E_BAD_ARGUMENT on null pointers, rows outside the frame, samples = 0 or
// parameters polaris_hip_set_denoise / polaris_hip_set_variance refuse (sigma_variance must be non-zero).
int polaris_host_variance(const float *frame_acc, uint32_t samples, const float *temporal, const float *prior2, const float *guide,
                          const float *albedo, uint32_t frame_w, uint32_t frame_h, uint32_t block_y, uint32_t block_h,
                          const PolarisDenoiseParams *p, const PolarisVarianceParams *v, float *out) {
	if (!frame_acc || !guide || !albedo || !out || (!temporal) != (!prior2) || samples == 0) return POLARIS_E_BAD_ARGUMENT;
	if (!params_ok(p, v) || !rows_ok(frame_w, frame_h, block_y, block_h)) return POLARIS_E_BAD_ARGUMENT;
	const uint32_t W = frame_w, y0 = block_y, y1 = block_y + block_h;
	const float n = (float)samples, weight = (float)(1.0 / (float)samples); // (polaris_hip_sync_framebuffer's)
	const DnIter it0 = dn_iter(0, p->normal_power_log2, p->sigma_depth, 0.0f);
	auto moments = [&](size_t j, float m[3]) {
		const float *a = frame_acc + 4 * j;
		float c[3] = {a[0] * weight, a[1] * weight, a[2] * weight};
		float pm = 0.0f, h2 = 0.0f;
		if (temporal) {
			for (int ch = 0; ch < 3; ch++) c[ch] = temporal[4 * j + ch];
			h2 = prior2[4 * j];
			pm = prior2[4 * j + 3];
		}
		va_moments(c, a[3], n, weight, pm, h2, m);
	};
	auto load = [&](uint32_t j, DnTap &t, float m[3]) -> bool {
		if (!dn_filtered(albedo[4 * (size_t)j + 3])) return false;
		const float *g = guide + 4 * (size_t)j;
		t = DnTap{g[0], g[1], g[2], g[3], 0.0f, 0.0f, 0.0f};
		moments(j, m);
		return true;
	};
	for (size_t i = (size_t)y0 * W; i < (size_t)y1 * W; i++) {
		float mi[3];
		moments(i, mi);
		float var = 0.0f;
		if (dn_filtered(albedo[4 * i + 3])) {
			const float *g = guide + 4 * i;
			const DnTap ci{g[0], g[1], g[2], g[3], 0.0f, 0.0f, 0.0f};
			var = va_estimate((uint32_t)(i % W), (uint32_t)(i / W), W, y0, y1, ci, mi, v->min_samples, it0, load);
		}
		float *o = out + 4 * i;
		o[0] = mi[0]; o[1] = mi[1]; o[2] = mi[2]; o[3] = var;
	}
	return POLARIS_OK;
}

// The variance-guided filter over the rows [block_y, block_y + block_h) of c = acc * weight (the TEMPORAL plane with weight 1 under
// temporal reuse) with the VARIANCE plane `variance`, into out (DENOISED: rgb | filtered variance; its other rows are not written).
// iterations = 0 passes c | 0 through.  POLARIS_E_BAD_ARGUMENT as polaris_host_variance.
int polaris_host_denoise_variance(const float *acc, float weight, const float *variance, const float *guide, const float *albedo, uint32_t frame_w,
                                  uint32_t frame_h, uint32_t block_y, uint32_t block_h, const PolarisDenoiseParams *p, const PolarisVarianceParams *v,
                                  float *out) {
	if (!acc || !variance || !guide || !albedo || !out) return POLARIS_E_BAD_ARGUMENT;
	if (!params_ok(p, v) || !rows_ok(frame_w, frame_h, block_y, block_h)) return POLARIS_E_BAD_ARGUMENT;
	const uint32_t W = frame_w, y0 = block_y, y1 = block_y + block_h;
	const size_t n = (size_t)block_h * W, base = (size_t)y0 * W;
	std::vector<float> cur(n * 4), nxt(n * 4); // r^k | v^k of the request's rows
	auto filtered = [&](size_t i) { return dn_filtered(albedo[4 * i + 3]); };
	for (size_t q = 0; q < n; q++) {
		const float *a = albedo + 4 * (base + q);
		for (int ch = 0; ch < 3; ch++) cur[4 * q + ch] = (acc[4 * (base + q) + ch] * weight) / dn_demod_albedo(a[ch]);
		cur[4 * q + 3] = va_demod(variance[4 * (base + q) + 3], a);
	}
	for (uint32_t k = 0; k < p->iterations; k++) {
		const DnIter it = dn_iter(k, p->normal_power_log2, p->sigma_depth, 0.0f);
		auto load = [&](uint32_t j, DnTap &t, float &vj) -> bool {
			if (!filtered(j)) return false;
			const float *g = guide + 4 * (size_t)j;
			const float *r = cur.data() + 4 * ((size_t)j - base);
			t = DnTap{g[0], g[1], g[2], g[3], r[0], r[1], r[2]};
			vj = r[3];
			return true;
		};
		for (size_t q = 0; q < n; q++) {
			const uint32_t i = (uint32_t)(base + q);
			if (!filtered(i)) continue;
			DnTap ci;
			float vi;
			(void)load(i, ci, vi);
			va_step(i % W, i / W, W, y0, y1, ci, vi, it, v->sigma_variance, load, nxt.data() + 4 * q);
		}
		for (size_t q = 0; q < n; q++)
			if (filtered(base + q)) for (int ch = 0; ch < 4; ch++) cur[4 * q + ch] = nxt[4 * q + ch];
	}
	for (size_t q = 0; q < n; q++) {
		const size_t i = base + q;
		float *o = out + 4 * i;
		const float *a = albedo + 4 * i;
		if (!filtered(i) || p->iterations == 0) {
			for (int ch = 0; ch < 3; ch++) o[ch] = acc[4 * i + ch] * weight;
			o[3] = 0.0f;
		} else {
			for (int ch = 0; ch < 3; ch++) o[ch] = cur[4 * q + ch] * dn_demod_albedo(a[ch]);
			o[3] = va_remod(cur[4 * q + 3], a);
		}
	}
	return POLARIS_OK;
}

} // extern "C"
