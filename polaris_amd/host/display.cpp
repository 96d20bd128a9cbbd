// display.cpp -- the CPU restatement of the display stage (kernels.h k_meter, k_expose, k_display), for the tests: the same arithmetic
// from polaris_amd/csrc/display.h in the same order, so the bytes, the histogram and the exposure of polaris_hip_display_planes and
// of a displayed polaris_hip_sync_framebuffer are compared with these bit for bit (tests/test_gpu_display.py), and their numbers are
// checked against an independent numpy statement of the algorithm (tests/test_display_cpu.py).
#include <cstring>

#include "display.h"
#include "polaris_hip.h"

using namespace pol;

namespace {
template <int OP, bool SRGB>
void display_rows(const float *plane, size_t first, size_t n, float weight, float exposure, float E, const DpCurve &k, uint8_t *rgba) {
	for (size_t i = first; i < first + n; i++) dp_pixel<OP, SRGB>(plane + 4 * i, weight, exposure, E, k, rgba + 4 * i);
}
template <int OP>
void display_rows(bool srgb, const float *plane, size_t first, size_t n, float weight, float exposure, float E, const DpCurve &k, uint8_t *rgba) {
	if (srgb) display_rows<OP, true>(plane, first, n, weight, exposure, E, k, rgba);
	else display_rows<OP, false>(plane, first, n, weight, exposure, E, k, rgba);
}
} // namespace

extern "C" {

// polaris_hip_display_planes on the CPU, argument for argument: the rows [block_y, block_y + block_h) of plane (W x H float4) metered
// with weight (p->auto_exposure), exposed from the state prev_log2E (null: none) and displayed into rgba, whose other rows are not
// written.  histogram (256 counts) and info may be null.  POLARIS_E_BAD_ARGUMENT as polaris_hip_display_planes.
int polaris_host_display(const float *plane, uint32_t W, uint32_t H, uint32_t block_y, uint32_t block_h, float weight, float exposure,
                         const PolarisDisplayParams *p, const float *prev_log2E, uint8_t *rgba, uint32_t *histogram, PolarisExposureInfo *info) {
	if (!plane || !rgba || !p || p->struct_size != sizeof(PolarisDisplayParams) || !p->enabled || dp_check(*p) || W == 0 || H == 0 ||
	    (uint64_t)W * H > (1ull << 26) || block_h == 0 || block_y >= H || block_h > H - block_y || (info && info->struct_size != sizeof(PolarisExposureInfo)))
		return POLARIS_E_BAD_ARGUMENT;
	const size_t first = (size_t)block_y * W, n = (size_t)block_h * W;
	uint32_t counts[kDpBins] = {};
	DpExposure s{};
	s.E = 1.0f;
	if (prev_log2E) { s.log2E = *prev_log2E; s.valid = 1u; }
	if (p->auto_exposure) {
		for (size_t i = first; i < first + n; i++) {
			const float *a = plane + 4 * i;
			const int b = dp_bin(dp_lum(a[0], a[1], a[2], weight));
			if (b >= 0) counts[b]++;
		}
		float value[kDpBins];
		for (uint32_t b = 0; b < kDpBins; b++) value[b] = dp_bin_value(b);
		dp_expose(counts, value, DpMeter{p->low_permille, p->high_permille, dp_log2_key(p->key), p->compensation_ev, p->min_ev, p->max_ev, p->adapt}, s);
	}
	const float E = p->auto_exposure ? s.E : 1.0f;
	const DpCurve k = dp_curve(p->white);
	const bool srgb = p->srgb != 0;
	switch (p->tone_operator) {
	case POLARIS_TONE_REINHARD_WHITE: display_rows<POLARIS_TONE_REINHARD_WHITE>(srgb, plane, first, n, weight, exposure, E, k, rgba); break;
	case POLARIS_TONE_ACES: display_rows<POLARIS_TONE_ACES>(srgb, plane, first, n, weight, exposure, E, k, rgba); break;
	case POLARIS_TONE_HABLE: display_rows<POLARIS_TONE_HABLE>(srgb, plane, first, n, weight, exposure, E, k, rgba); break;
	default: display_rows<POLARIS_TONE_REINHARD>(srgb, plane, first, n, weight, exposure, E, k, rgba); break;
	}
	if (histogram) memcpy(histogram, counts, sizeof counts);
	if (info) *info = PolarisExposureInfo{sizeof(PolarisExposureInfo), s.valid, (uint64_t)s.n_hi << 32 | s.n_lo, s.avg, s.log2E, s.E, 0};
	return POLARIS_OK;
}

} // extern "C"
