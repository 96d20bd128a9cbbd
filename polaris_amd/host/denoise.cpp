// denoise.cpp -- the CPU restatement of the denoiser's filter (kernels.h k_denoise), for the tests: the same per-pixel
// arithmetic from polaris_amd/csrc/denoise.h, the same iteration order, so the DENOISED plane of polaris_hip_sync_framebuffer
// is compared with this bit for bit (tests/test_gpu_denoise.py), and its numbers are checked against an independent numpy
// statement of the algorithm (tests/test_denoise_cpu.py).
#include <cstring>
#include <vector>

#include "denoise.h"
#include "polaris_hip.h"

using namespace pol;

extern "C" {

// frame_acc, guide, albedo, out: frame_w * frame_h float4 (row-major).  Filters the rows [block_y, block_y + block_h) of the
// running mean frame_acc * weight into `out`; the other rows of `out` are not written.  POLARIS_E_BAD_ARGUMENT on null
// pointers, rows outside the frame or parameters polaris_hip_set_denoise refuses; iterations = 0 passes c through.
int polaris_host_denoise(const float *frame_acc, float weight, const float *guide, const float *albedo, uint32_t frame_w, uint32_t frame_h,
                         uint32_t block_y, uint32_t block_h, const PolarisDenoiseParams *p, float *out) {
	if (!frame_acc || !guide || !albedo || !p || !out) return POLARIS_E_BAD_ARGUMENT;
	if (p->struct_size != sizeof(PolarisDenoiseParams)) return POLARIS_E_BAD_ARGUMENT;
	if (dn_check(p->iterations, p->normal_power_log2, p->sigma_depth, p->sigma_luminance)) return POLARIS_E_BAD_ARGUMENT;
	if (frame_w == 0 || frame_h == 0 || block_h == 0 || (uint64_t)block_y + block_h > frame_h) return POLARIS_E_BAD_ARGUMENT;
	const uint32_t W = frame_w, y0 = block_y, y1 = block_y + block_h;
	const size_t n = (size_t)block_h * W, base = (size_t)y0 * W;
	std::vector<float> cur(n * 3), nxt(n * 3); // r^k of the request's rows
	auto c = [&](size_t i, int ch) { return frame_acc[4 * i + ch] * weight; };
	auto filtered = [&](size_t i) { return dn_filtered(albedo[4 * i + 3]); };
	for (size_t q = 0; q < n; q++)
		for (int ch = 0; ch < 3; ch++) cur[3 * q + ch] = c(base + q, ch) / dn_demod_albedo(albedo[4 * (base + q) + ch]);
	for (uint32_t k = 0; k < p->iterations; k++) {
		const DnIter it = dn_iter(k, p->normal_power_log2, p->sigma_depth, p->sigma_luminance);
		auto load = [&](uint32_t j, DnTap &t) -> bool {
			if (!filtered(j)) return false;
			const float *g = guide + 4 * (size_t)j;
			const float *r = cur.data() + 3 * ((size_t)j - base);
			t = DnTap{g[0], g[1], g[2], g[3], r[0], r[1], r[2]};
			return true;
		};
		for (size_t q = 0; q < n; q++) {
			const uint32_t i = (uint32_t)(base + q);
			if (!filtered(i)) continue;
			DnTap ci;
			(void)load(i, ci);
			dn_step(i % W, i / W, W, y0, y1, ci, it, load, nxt.data() + 3 * q);
		}
		for (size_t q = 0; q < n; q++)
			if (filtered(base + q)) for (int ch = 0; ch < 3; ch++) cur[3 * q + ch] = nxt[3 * q + ch];
	}
	for (size_t q = 0; q < n; q++) {
		const size_t i = base + q;
		float *o = out + 4 * i;
		if (!filtered(i) || p->iterations == 0) {
			for (int ch = 0; ch < 3; ch++) o[ch] = c(i, ch);
		} else {
			for (int ch = 0; ch < 3; ch++) o[ch] = cur[3 * q + ch] * dn_demod_albedo(albedo[4 * i + ch]);
		}
		o[3] = 0.0f;
	}
	return POLARIS_OK;
}

} // extern "C"
