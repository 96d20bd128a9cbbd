// display.h -- the arithmetic of the display stage polaris_hip_sync_framebuffer runs when polaris_hip_set_display turns it on
// (include/polaris_hip.h): the luminance histogram's binning, the exposure a histogram implies, the tone curves and
// the transfer functions.
//
// ONE definition for both sides, as denoise.h / temporal.h / variance.h: the HIP kernels (kernels.h, k_meter, k_expose, k_display)
// and the CPU restatement the tests compare them with (polaris_amd/host/display.cpp) include this header, and both are compiled
// without FMA contraction and with IEEE division, so the two agree bit for bit.  The two values that need a logarithm of a
// parameter -- the bins' log2 values and log2(key) -- are computed on the host in double and handed to both sides as floats.
#pragma once

#include <stdint.h>

#include "polaris_hip.h"
#include "polaris_math.h"
#include "variance.h"

#include <cmath>

namespace pol {

constexpr uint32_t kDpBins = 256;            // 8 bins an octave over [2^-16, 2^16)
constexpr int kDpMinExp = -16;               // the first bin's octave
constexpr uint32_t kDpFirstBits = (uint32_t)(127 + kDpMinExp) << 23; // the bits of 2^-16: the least metered luminance
constexpr float kDpMaxEv = 24.0f;            // min_ev, max_ev, compensation_ev within [-this, this] (pm_exp's range is 128 octaves)
constexpr float kDpMinWhite = 1e-3f, kDpMaxWhite = 1e6f, kDpMinKey = 1e-6f, kDpMaxKey = 1e6f;
constexpr float kDpLn2 = 0.69314718055994530942f;

// The metered luminance of a pixel: the plane's rgb times the sync's weight, without the request's exposure.
PM_HD float dp_lum(float r, float g, float b, float weight) { return va_lum(r * weight, g * weight, b * weight); }

// The bin of luminance L from its bits alone: -1 = not metered (L < 2^-16, negative, NaN or infinite); else the exponent and the top
// three mantissa bits counted from 2^-16, L >= 2^16 in the last bin.
PM_HD int dp_bin(float L) {
	const uint32_t u = pm_f2u(L);
	if (u < kDpFirstBits || u >= 0x7f800000u) return -1; // (a set sign bit is above 0x7f800000)
	const uint32_t b = (u >> 20) - (kDpFirstBits >> 20);
	return (int)(b < kDpBins ? b : kDpBins - 1);
}

// Host only: the log2 value of bin b = 8 (e + 16) + k, e + log2(1 + (k + 1/2) / 8) in double rounded to float, and log2(key).
inline float dp_bin_value(uint32_t b) { return (float)((double)((int)(b >> 3) + kDpMinExp) + std::log2(1.0 + ((double)(b & 7u) + 0.5) / 8.0)); }
inline float dp_log2_key(float key) { return (float)std::log2((double)key); }

// What k_expose needs of PolarisDisplayParams.
struct DpMeter {
	uint32_t low_permille, high_permille;
	float log2_key, compensation_ev, min_ev, max_ev, adapt;
};
// The exposure state (log2E | valid) with what the last k_expose read and computed.
struct DpExposure {
	float log2E;
	uint32_t valid; // a metered sync has set log2E since the last reset
	float E;        // the exposure the display step multiplies by
	float avg;      // the window's mean log2 luminance (0 with nothing metered)
	uint32_t n_lo, n_hi; // the metered pixel count (64 bits)
};

// The exposure of one sync from the 256 counts, in three steps that the kernel and the restatement both take:
//   dp_window: N = sum of the counts; the window is the pixels of rank [lo, hi) in ascending luminance, lo = N low / 1000,
//   hi = max(N high / 1000, lo + 1) in 64-bit integers.
//   dp_window_count: bin b with the ranks [cum, cum + c) holds n_b = |[cum, cum + c) ^ [lo, hi)| of them; its term is (float)n_b * value[b].
//   dp_exposure: sum = the 256 terms added in ascending bins to one running float (a term of an empty bin is a zero and changes nothing);
//   avg = sum / (float)(hi - lo); target = clamp((log2_key - avg) + compensation_ev, min_ev, max_ev); log2E = target without a state,
//   else log2E + (target - log2E) * adapt; E = pm_exp(log2E * ln 2).  N = 0: the state stays, E = exp2(log2E) with a state, 1 without.
PM_HD void dp_window(uint64_t N, const DpMeter &m, uint64_t &lo, uint64_t &hi) {
	lo = N * m.low_permille / 1000u;
	hi = N * m.high_permille / 1000u;
	if (hi < lo + 1) hi = lo + 1;
}
PM_HD float dp_window_term(uint64_t cum, uint32_t c, uint64_t lo, uint64_t hi, float value) {
	const uint64_t end = cum + c;
	const uint64_t a = cum > lo ? cum : lo, z = end < hi ? end : hi;
	return (float)(z > a ? z - a : 0u) * value;
}
PM_HD void dp_exposure(uint64_t N, uint64_t lo, uint64_t hi, const float *term, const DpMeter &m, DpExposure &s) {
	s.n_lo = (uint32_t)N;
	s.n_hi = (uint32_t)(N >> 32);
	if (N == 0) {
		s.avg = 0.0f;
		s.E = s.valid ? pm_exp(s.log2E * kDpLn2) : 1.0f;
		return;
	}
	float sum = 0.0f;
	for (uint32_t b = 0; b < kDpBins; b++) sum += term[b];
	s.avg = sum / (float)(hi - lo);
	const float target = pm_clamp((m.log2_key - s.avg) + m.compensation_ev, m.min_ev, m.max_ev);
	s.log2E = s.valid ? s.log2E + (target - s.log2E) * m.adapt : target;
	s.valid = 1u;
	s.E = pm_exp(s.log2E * kDpLn2);
}
// The three steps in a row (the restatement; k_expose takes the first two with a wave, kernels.h).
inline void dp_expose(const uint32_t *counts, const float *value, const DpMeter &m, DpExposure &s) {
	uint64_t N = 0, lo = 0, hi = 1, cum = 0;
	for (uint32_t b = 0; b < kDpBins; b++) N += counts[b];
	if (N) dp_window(N, m, lo, hi);
	float term[kDpBins];
	for (uint32_t b = 0; b < kDpBins; b++) {
		term[b] = dp_window_term(cum, counts[b], lo, hi, value[b]);
		cum += counts[b];
	}
	dp_exposure(N, lo, hi, term, m, s);
}

// The tone curve's constants: white^2 (REINHARD_WHITE) and the Hable curve's value at white.
struct DpCurve {
	float w2, hable_white;
};
// John Hable's Uncharted 2 curve with its published constants A .. F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30 (no exposure bias).
PM_HD float dp_hable(float x) { return (x * (0.15f * x + 0.05f) + 0.004f) / (x * (0.15f * x + 0.50f) + 0.06f) - 0.02f / 0.30f; }
PM_HD DpCurve dp_curve(float white) { return DpCurve{white * white, dp_hable(white)}; }

// One channel through tone operator OP: c = radiance * weight * exposure * E.
template <int OP>
PM_HD float dp_tone(float c, const DpCurve &k) {
	if (OP == POLARIS_TONE_REINHARD_WHITE) return (c * (1.0f + c / k.w2)) / (1.0f + c);
	if (OP == POLARIS_TONE_ACES) return (c * (2.51f * c + 0.03f)) / (c * (2.43f * c + 0.59f) + 0.14f); // Narkowicz 2015
	if (OP == POLARIS_TONE_HABLE) return dp_hable(c) / k.hable_white;
	return c / (c + 1.0f); // POLARIS_TONE_REINHARD: tonemapSimpleReinhard (kernels/hdr.cl:20)
}
// The transfer function: the reference's pow(1 / 2.2), or the piecewise sRGB OETF.
template <bool SRGB>
PM_HD float dp_transfer(float m) {
	if (!SRGB) return pm_pow(m, 1.0f / 2.2f);
	return m <= 0.0031308f ? 12.92f * m : 1.055f * pm_pow(m, 1.0f / 2.4f) - 0.055f;
}
// The byte of one channel: clamped to [0, 1], times 255, truncated (kernels.h tonemap_byte); a NaN is 0.
template <int OP, bool SRGB>
PM_HD uint8_t dp_byte(float c, const DpCurve &k) {
	const float v = pm_clamp(dp_transfer<SRGB>(dp_tone<OP>(c, k)), 0.0f, 1.0f) * 255.0f;
	return v >= 0.0f ? (uint8_t)v : (uint8_t)0;
}
// The four bytes of a pixel: rgb * weight * exposure * E per channel, in this order, alpha 255.
template <int OP, bool SRGB>
PM_HD void dp_pixel(const float rgb[3], float weight, float exposure, float E, const DpCurve &k, uint8_t out[4]) {
	for (int ch = 0; ch < 3; ch++) out[ch] = dp_byte<OP, SRGB>(rgb[ch] * weight * exposure * E, k);
	out[3] = 255;
}

// Parameter check shared by polaris_hip_set_display, polaris_hip_display_planes and the host restatement: 0 = valid.  Off
// (enabled = 0) is valid whatever the other fields hold.
PM_HD bool dp_within(float x, float lo, float hi) { return x >= lo && x <= hi; } // (false for a NaN)
PM_HD int dp_check(const PolarisDisplayParams &p) {
	if (p.enabled > 1) return 1;
	if (!p.enabled) return 0;
	if (p.tone_operator > POLARIS_TONE_HABLE || p.srgb > 1 || p.auto_exposure > 1) return 1;
	if (!dp_within(p.white, kDpMinWhite, kDpMaxWhite)) return 1;
	if (!p.auto_exposure) return 0;
	if (!dp_within(p.key, kDpMinKey, kDpMaxKey) || !dp_within(p.compensation_ev, -kDpMaxEv, kDpMaxEv)) return 1;
	if (p.high_permille > 1000 || p.low_permille >= p.high_permille) return 1;
	if (!dp_within(p.min_ev, -kDpMaxEv, kDpMaxEv) || !dp_within(p.max_ev, p.min_ev, kDpMaxEv)) return 1;
	if (!(p.adapt > 0.0f && p.adapt <= 1.0f)) return 1;
	return 0;
}

} // namespace pol
