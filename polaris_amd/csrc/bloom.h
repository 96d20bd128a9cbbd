// bloom.h -- the arithmetic of the bloom the display stage adds when polaris_hip_set_bloom turns it on (include/polaris_hip.h;
// DESIGN.md 10m): the bright pass, the 4 x 4 downsample, the 2 x tent upsample, the pyramid's geometry and the parameter check.
//
// ONE definition for both sides, as display.h: the HIP kernels (kernels.h, k_bloom_down, k_bloom_up, k_bloom_tail, k_display_bloom)
// and the CPU restatement (polaris_amd/host/bloom.cpp) include this header, both compiled without FMA contraction, so the two agree
// bit for bit.  Every function takes its source as a callable `src(x, y, out[4])` that is handed clamped coordinates, so global
// memory, a staged LDS tile and a host array run the same expression in the same order.
#pragma once

#include <stdint.h>

#include "display.h"
#include "polaris_hip.h"
#include "polaris_math.h"
#include "variance.h"

namespace pol {

constexpr uint32_t kBlMaxLevels = 8;
constexpr float kBlMaxValue = 65536.0f; // a bright-passed channel is within [0, this]: every later sum stays finite
constexpr float kBlMaxThreshold = 65536.0f, kBlMaxIntensity = 16.0f;
constexpr float kBlEps = 1e-5f;
constexpr uint32_t kBlTailPixels = 1024; // k_bloom_tail starts at the first level with at most this many pixels ...
constexpr uint32_t kBlTailLds = 2112;    // ... and holds that level and every coarser one in this many float4 of LDS

// The pyramid over a region w[0] x h[0]: level l >= 1 is (w[l-1] + 1) / 2 x (h[l-1] + 1) / 2; L = min(levels asked for, the first
// level that is one pixel), at least 1.  off[l]: where level l >= 1 starts in the pyramid's one allocation of off[L + 1] float4.
struct BlLevels {
	uint32_t L;
	uint32_t w[kBlMaxLevels + 1], h[kBlMaxLevels + 1], off[kBlMaxLevels + 2];
};
PM_HD BlLevels bl_levels(uint32_t W, uint32_t rows, uint32_t levels) {
	BlLevels g{};
	g.w[0] = W;
	g.h[0] = rows;
	g.L = 0;
	uint32_t at = 0;
	for (uint32_t l = 1; l <= kBlMaxLevels; l++) {
		g.w[l] = (g.w[l - 1] + 1) / 2;
		g.h[l] = (g.h[l - 1] + 1) / 2;
		g.off[l] = at;
		at += g.w[l] * g.h[l];
		g.L = l;
		if (l >= levels || (g.w[l] == 1 && g.h[l] == 1)) break;
	}
	g.off[g.L + 1] = at;
	return g;
}
// The first level k_bloom_tail takes: the first with at most kBlTailPixels pixels whose level and coarser ones fit kBlTailLds; L + 1: none.
PM_HD uint32_t bl_tail_start(const BlLevels &g) {
	for (uint32_t l = 1; l <= g.L; l++)
		if (g.w[l] * g.h[l] <= kBlTailPixels && g.off[g.L + 1] - g.off[l] <= kBlTailLds) return l;
	return g.L + 1;
}

// What the bright pass needs of a sync and of PolarisBloomParams.
struct BlBright {
	float weight, exposure, E, threshold, knee;
};
// The bright pass of one source pixel: c = ((rgb * weight) * exposure) * E per channel (display.h dp_pixel's expression); a channel that
// is NaN or not above 0 becomes 0, one above kBlMaxValue becomes kBlMaxValue; m = max(r, g, b), k = threshold * knee,
// s = clamp((m - threshold) + k, 0, 2 k), s = (s * s) / (4 k + 1e-5); b = c * (max(s, m - threshold) / max(m, 1e-5)).
// KARIS: out[3] = 1 / (1 + va_lum(b)), the tap's weight in the first downsample; else out[3] = 0.
template <bool KARIS>
PM_HD void bl_bright(const float rgb[3], const BlBright &p, float out[4]) {
	float c[3];
	for (int ch = 0; ch < 3; ch++) {
		const float v = rgb[ch] * p.weight * p.exposure * p.E;
		c[ch] = v > 0.0f ? (v > kBlMaxValue ? kBlMaxValue : v) : 0.0f; // (false for a NaN)
	}
	float m = c[0] > c[1] ? c[0] : c[1];
	m = m > c[2] ? m : c[2];
	const float k = p.threshold * p.knee;
	float s = pm_clamp((m - p.threshold) + k, 0.0f, 2.0f * k);
	s = (s * s) / (4.0f * k + kBlEps);
	const float f = pm_max(s, m - p.threshold) / pm_max(m, kBlEps);
	for (int ch = 0; ch < 3; ch++) out[ch] = c[ch] * f;
	out[3] = KARIS ? 1.0f / (1.0f + va_lum(out[0], out[1], out[2])) : 0.0f;
}

PM_HD float bl_k(int i) { return i == 0 || i == 3 ? 0.125f : 0.375f; } // {1, 3, 3, 1} / 8
PM_HD int bl_clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// D(x, y) of a level from the level below (sw x sh; level 1: the bright pass): over j = 0..3 (outer) and i = 0..3 (inner)
// K[j] * (running row sum of K[i] * src(2 x - 1 + i, 2 y - 1 + j)), coordinates clamped to the source's extent.  KARIS (level 1
// only): every tap is weighted by its src[3] and the sum is divided by the same sum of the weights.  out[3] = 0.
template <bool KARIS, class Src>
PM_HD void bl_down(const Src &src, int x, int y, int sw, int sh, float out[4]) {
	float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	for (int j = 0; j < 4; j++) {
		const int sy = bl_clampi(2 * y - 1 + j, sh);
		float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
		for (int i = 0; i < 4; i++) {
			float t[4];
			src(bl_clampi(2 * x - 1 + i, sw), sy, t);
			if (KARIS) {
				for (int ch = 0; ch < 3; ch++) row[ch] += bl_k(i) * (t[ch] * t[3]);
				row[3] += bl_k(i) * t[3];
			} else
				for (int ch = 0; ch < 3; ch++) row[ch] += bl_k(i) * t[ch];
		}
		for (int ch = 0; ch < 4; ch++) acc[ch] += bl_k(j) * row[ch];
	}
	for (int ch = 0; ch < 3; ch++) out[ch] = KARIS ? acc[ch] / acc[3] : acc[ch];
	out[3] = 0.0f;
}

// The 2 x tent: fine index i takes coarse a and a + 1 with weights wa, 1 - wa: even i: a = (i >> 1) - 1, 1/4 | 3/4; odd i: a = i >> 1,
// 3/4 | 1/4; both clamped to the coarse extent n.
PM_HD void bl_tent(int i, int n, int &a, int &b, float &wa, float &wb) {
	const int h = i >> 1;
	if (i & 1) { a = h; b = h + 1; wa = 0.75f; wb = 0.25f; }
	else { a = h - 1; b = h; wa = 0.25f; wb = 0.75f; }
	a = bl_clampi(a, n);
	b = bl_clampi(b, n);
}
// up(U)(x, y) of a coarse level cw x ch: x inside y -- wya * (wxa * U(xa, ya) + wxb * U(xb, ya)) + wyb * (wxa * U(xa, yb) + wxb * U(xb, yb)).
template <class Src>
PM_HD void bl_up(const Src &src, int x, int y, int cw, int ch, float out[3]) {
	int xa, xb, ya, yb;
	float wxa, wxb, wya, wyb;
	bl_tent(x, cw, xa, xb, wxa, wxb);
	bl_tent(y, ch, ya, yb, wya, wyb);
	float p[4], q[4], r[4], s[4];
	src(xa, ya, p);
	src(xb, ya, q);
	src(xa, yb, r);
	src(xb, yb, s);
	for (int c = 0; c < 3; c++) out[c] = wya * (wxa * p[c] + wxb * q[c]) + wyb * (wxa * r[c] + wxb * s[c]);
}
// U_l(x, y) = D_l(x, y) + up(U_{l+1})(x, y)
template <class Src>
PM_HD void bl_merge(const float d[4], const Src &coarse, int x, int y, int cw, int ch, float out[4]) {
	float u[3];
	bl_up(coarse, x, y, cw, ch, u);
	for (int c = 0; c < 3; c++) out[c] = d[c] + u[c];
	out[3] = 0.0f;
}
// The full-resolution term of pixel (x, y): up(U_1)(x, y) / (float)L per channel.
template <class Src>
PM_HD void bl_term(const Src &u1, int x, int y, int w1, int h1, uint32_t L, float out[3]) {
	bl_up(u1, x, y, w1, h1, out);
	for (int c = 0; c < 3; c++) out[c] = out[c] / (float)L;
}
// The four bytes of a bloomed pixel: c = rgb * weight * exposure * E as dp_pixel, then c + intensity * term through dp_byte.
template <int OP, bool SRGB>
PM_HD void bl_pixel(const float rgb[3], const float term[3], float weight, float exposure, float E, float intensity, const DpCurve &k, uint8_t out[4]) {
	for (int ch = 0; ch < 3; ch++) out[ch] = dp_byte<OP, SRGB>(rgb[ch] * weight * exposure * E + intensity * term[ch], k);
	out[3] = 255;
}

// Parameter check shared by polaris_hip_set_bloom, polaris_hip_bloom_planes and the host restatement: 0 = valid.  Off (enabled = 0) is
// valid whatever the fields after karis hold.
PM_HD int bl_check(const PolarisBloomParams &p) {
	if (p.enabled > 1 || p.karis > 1) return 1;
	if (!p.enabled) return 0;
	if (p.levels < 1 || p.levels > kBlMaxLevels) return 1;
	if (!dp_within(p.threshold, 0.0f, kBlMaxThreshold) || !dp_within(p.knee, 0.0f, 1.0f) || !dp_within(p.intensity, 0.0f, kBlMaxIntensity)) return 1;
	return 0;
}

} // namespace pol
