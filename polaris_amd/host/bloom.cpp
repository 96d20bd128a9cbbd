// bloom.cpp -- the CPU restatement of the bloom of the display stage (kernels.h k_bloom_down, k_bloom_up, k_bloom_tail,
// k_display_bloom), for the tests: the same arithmetic from polaris_amd/csrc/bloom.h in the same order, level by level over whole
// planes, so the bytes and U_1 of polaris_hip_bloom_planes and of a bloomed polaris_hip_sync_framebuffer are compared with these bit
// for bit (tests/test_gpu_bloom.py), and their numbers are checked against an independent numpy statement (tests/test_bloom_cpu.py).
#include <cstring>
#include <vector>

#include "bloom.h"
#include "polaris_hip.h"

using namespace pol;

extern "C" int polaris_host_display(const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight, float exposure,
                                    const PolarisDisplayParams *p, const float *prev_log2E, uint8_t *rgba, uint32_t *histogram, PolarisExposureInfo *info);

namespace {
struct Plane { // a level, or the source rows: w floats-of-four wide
	const float *p; int w;
	void operator()(int x, int y, float t[4]) const { for (int c = 0; c < 4; c++) t[c] = p[4 * ((size_t)y * w + x) + c]; }
};
template <bool KARIS>
struct BrightPlane {
	const float *p; int w; BlBright b;
	void operator()(int x, int y, float t[4]) const { bl_bright<KARIS>(p + 4 * ((size_t)y * w + x), b, t); }
};
template <int OP, bool SRGB>
void display_rows(const float *src, const float *term, size_t n, float weight, float exposure, float E, float intensity, const DpCurve &k, uint8_t *rgba) {
	for (size_t i = 0; i < n; i++) bl_pixel<OP, SRGB>(src + 4 * i, term + 4 * i, weight, exposure, E, intensity, k, rgba + 4 * i);
}
template <int OP>
void display_rows(bool srgb, const float *src, const float *term, size_t n, float weight, float exposure, float E, float intensity, const DpCurve &k, uint8_t *rgba) {
	if (srgb) display_rows<OP, true>(src, term, n, weight, exposure, E, intensity, k, rgba);
	else display_rows<OP, false>(src, term, n, weight, exposure, E, intensity, k, rgba);
}
} // namespace

extern "C" {

// The shared parameter check (bloom.h bl_check) with polaris_hip_set_bloom's struct_size rule: 0 = accepted.
int polaris_host_bloom_check(const PolarisBloomParams *p) { return !p || p->struct_size != sizeof(PolarisBloomParams) || bl_check(*p); }

// The levels used over a region W x rows with `levels` asked for; w1, h1 (may be null): level 1's extent.
uint32_t polaris_host_bloom_levels(uint32_t W, uint32_t rows, uint32_t levels, uint32_t *w1, uint32_t *h1) {
	const BlLevels g = bl_levels(W, rows, levels);
	if (w1) *w1 = g.w[1];
	if (h1) *h1 = g.h[1];
	return g.L;
}

// polaris_hip_bloom_planes on the CPU, argument for argument, plus term (may be null): the full-resolution bloom term up(U_1) / L of the
// request's rows, block_h x W x 4 floats (rgb | 0).  level1 (may be null): U_1, h_1 x w_1 x 4 floats.  rgba's other rows are not written.
// POLARIS_E_BAD_ARGUMENT as polaris_hip_bloom_planes.
int polaris_host_bloom(const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight, float exposure,
                       const PolarisDisplayParams *dp, const PolarisBloomParams *bp, const float *prev_log2E, uint8_t *rgba, float *level1, float *term,
                       uint32_t *levels_used) {
	if (!bp || bp->struct_size != sizeof(PolarisBloomParams) || !bp->enabled || bl_check(*bp)) return POLARIS_E_BAD_ARGUMENT;
	PolarisExposureInfo info{};
	info.struct_size = sizeof info;
	// the display stage without bloom: checks the other arguments, meters, and writes bytes the bloomed ones below replace
	if (int rc = polaris_host_display(plane, W, H, block_y, block_h, weight, exposure, dp, prev_log2E, rgba, nullptr, &info)) return rc;
	const float E = dp->auto_exposure ? info.E : 1.0f;
	const float *src = plane + 4 * (size_t)block_y * W;
	const BlLevels g = bl_levels(W, block_h, bp->levels);
	std::vector<float> pyr(4 * (size_t)g.off[g.L + 1]);
	auto level = [&](uint32_t l) { return pyr.data() + 4 * (size_t)g.off[l]; };
	const BlBright bright{weight, exposure, E, bp->threshold, bp->knee};
	for (uint32_t l = 1; l <= g.L; l++)
		for (int y = 0; y < (int)g.h[l]; y++)
			for (int x = 0; x < (int)g.w[l]; x++) {
				float *o = level(l) + 4 * ((size_t)y * g.w[l] + x);
				const int sw = (int)g.w[l - 1], sh = (int)g.h[l - 1];
				if (l > 1) bl_down<false>(Plane{level(l - 1), sw}, x, y, sw, sh, o);
				else if (bp->karis) bl_down<true>(BrightPlane<true>{src, sw, bright}, x, y, sw, sh, o);
				else bl_down<false>(BrightPlane<false>{src, sw, bright}, x, y, sw, sh, o);
			}
	for (uint32_t l = g.L - 1; l >= 1; l--)
		for (int y = 0; y < (int)g.h[l]; y++)
			for (int x = 0; x < (int)g.w[l]; x++) {
				float *o = level(l) + 4 * ((size_t)y * g.w[l] + x);
				const float d[4] = {o[0], o[1], o[2], o[3]};
				bl_merge(d, Plane{level(l + 1), (int)g.w[l + 1]}, x, y, (int)g.w[l + 1], (int)g.h[l + 1], o);
			}
	const size_t n = (size_t)block_h * W;
	std::vector<float> full(4 * n, 0.0f);
	for (int y = 0; y < (int)block_h; y++)
		for (int x = 0; x < (int)W; x++) bl_term(Plane{level(1), (int)g.w[1]}, x, y, (int)g.w[1], (int)g.h[1], g.L, full.data() + 4 * ((size_t)y * W + x));
	const DpCurve k = dp_curve(dp->white);
	const bool srgb = dp->srgb != 0;
	uint8_t *out = rgba + 4 * (size_t)block_y * W;
	switch (dp->tone_operator) {
	case POLARIS_TONE_REINHARD_WHITE: display_rows<POLARIS_TONE_REINHARD_WHITE>(srgb, src, full.data(), n, weight, exposure, E, bp->intensity, k, out); break;
	case POLARIS_TONE_ACES: display_rows<POLARIS_TONE_ACES>(srgb, src, full.data(), n, weight, exposure, E, bp->intensity, k, out); break;
	case POLARIS_TONE_HABLE: display_rows<POLARIS_TONE_HABLE>(srgb, src, full.data(), n, weight, exposure, E, bp->intensity, k, out); break;
	default: display_rows<POLARIS_TONE_REINHARD>(srgb, src, full.data(), n, weight, exposure, E, bp->intensity, k, out); break;
	}
	if (level1) memcpy(level1, level(1), 4 * sizeof(float) * (size_t)g.w[1] * g.h[1]);
	if (term) memcpy(term, full.data(), 4 * sizeof(float) * n);
	if (levels_used) *levels_used = g.L;
	return POLARIS_OK;
}

} // extern "C"
