// denoise.h -- per-pixel arithmetic of the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) that
// polaris_hip_sync_framebuffer runs when denoising is on (include/polaris_hip.h, polaris_hip_set_denoise).
//
// ONE definition for both sides: the HIP kernel (kernels.h, k_denoise) and the CPU restatement the tests compare it with
// (polaris_amd/host/denoise.cpp) include this header, and both are compiled without FMA contraction and with IEEE division,
// so the two agree bit for bit.  Plain floats only: no HIP vector types, no host-only library calls.
//
// Inputs per pixel: c = frame accumulator rgb * weight (the running mean sync tone-maps), the GUIDE plane (first-hit shading
// normal xyz | hit distance) and the ALBEDO plane (first-hit reflectance rgb | leaf type bits, -1 = miss).  A pixel is FILTERED
// when its first hit exists and is not an emitter; every other pixel passes through unchanged and is never a tap.
#pragma once

#include <stdint.h>

#include "polaris_math.h"
#include "polaris_types.h"

namespace pol {

constexpr float kDnMinAlbedo = 1e-3f;   // demodulation floor per channel (black albedo would divide by zero)
constexpr uint32_t kDnMaxIterations = 8, kDnMaxNormalPowerLog2 = 10;
constexpr float kDnSigmaMin = 1e-6f, kDnSigmaMax = 1e6f; // a non-zero sigma outside this range makes a denominator underflow or the term vanish

// What one tap contributes: its guide and its demodulated radiance.
struct DnTap { float nx, ny, nz, t, r, g, b; };

// Arguments of one iteration k (step s = 1 << k), derived once on the host side of either implementation.
struct DnIter {
	uint32_t step;        // s
	uint32_t normal_pow;  // P: w_n = max(0, n_i . n_j)^(2^P) by P squarings
	float depth_scale;    // sigma_z * s  (0 = depth term off)
	float lum_scale;      // sigma_l^2 * 2^-k  (0 = luminance term off)
};

PM_HD DnIter dn_iter(uint32_t k, uint32_t normal_power_log2, float sigma_depth, float sigma_luminance) {
	DnIter it;
	it.step = 1u << k;
	it.normal_pow = normal_power_log2;
	it.depth_scale = sigma_depth * (float)it.step;
	it.lum_scale = (sigma_luminance * sigma_luminance) * pm_u2f((uint32_t)(127 - (int32_t)k) << 23); // * 2^-k, exact
	return it;
}

// The leaf word of the ALBEDO plane: filtered = a hit whose leaf is not EMISSIVE.
PM_HD bool dn_filtered(float albedo_w) {
	const uint32_t leaf = pm_f2u(albedo_w);
	return leaf != 0xFFFFFFFFu && leaf != POLARIS_BXDF_EMISSIVE;
}

PM_HD float dn_demod_albedo(float a) { return pm_max(a, kDnMinAlbedo); }

// B3 spline taps {1/16, 1/4, 3/8, 1/4, 1/16}, index 0..4
PM_HD float dn_h(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

PM_HD float dn_map(float x) { return x / (x + 1.0f); } // tone-mapped radiance for the luminance term

// Weight of tap j for centre i (j != i): h * w_n * w_z * w_l, left to right.
PM_HD float dn_weight(float h, const DnTap &ci, const DnTap &cj, const DnIter &it) {
	float wn = pm_max(0.0f, ci.nx * cj.nx + ci.ny * cj.ny + ci.nz * cj.nz);
	for (uint32_t p = 0; p < it.normal_pow; p++) wn = wn * wn;
	float wz = 1.0f;
	if (it.depth_scale != 0.0f) wz = pm_exp(-pm_fabs(ci.t - cj.t) / (it.depth_scale * ci.t));
	float wl = 1.0f;
	if (it.lum_scale != 0.0f) {
		const float dr = dn_map(ci.r) - dn_map(cj.r), dg = dn_map(ci.g) - dn_map(cj.g), db = dn_map(ci.b) - dn_map(cj.b);
		wl = pm_exp(-(dr * dr + dg * dg + db * db) / it.lum_scale);
	}
	return h * wn * wz * wl;
}

// One a-trous iteration for the filtered pixel (x, y): the 5 x 5 taps at stride s, dy outer, dx inner.  A tap outside the rows
// [y0, y1) or the frame width, or one that is not filtered, is skipped (not clamped).  The centre tap weighs h = 9/64 exactly
// (every term of a pixel against itself is 1), so the sum of weights is never 0.  load(j, tap) fills tap j and returns whether
// it is filtered.  Returns r^{k+1}_i in out[3].
template <class Load>
PM_HD void dn_step(uint32_t x, uint32_t y, uint32_t W, uint32_t y0, uint32_t y1, const DnTap &ci, const DnIter &it, Load load, float out[3]) {
	float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
	const int s = (int)it.step;
	for (int dy = -2; dy <= 2; dy++) {
		const int yy = (int)y + dy * s;
		if (yy < (int)y0 || yy >= (int)y1) continue;
		for (int dx = -2; dx <= 2; dx++) {
			const int xx = (int)x + dx * s;
			if (xx < 0 || xx >= (int)W) continue;
			const float h = dn_h(dx + 2) * dn_h(dy + 2);
			float w;
			DnTap cj;
			if (dx == 0 && dy == 0) {
				w = h;
				cj = ci;
			} else {
				if (!load((uint32_t)yy * W + (uint32_t)xx, cj)) continue;
				w = dn_weight(h, ci, cj, it);
			}
			sw += w;
			ar += w * cj.r;
			ag += w * cj.g;
			ab += w * cj.b;
		}
	}
	out[0] = ar / sw;
	out[1] = ag / sw;
	out[2] = ab / sw;
}

// Parameter check shared by polaris_hip_set_denoise and polaris_host_denoise: 0 = valid.
PM_HD bool dn_sigma_ok(float s) { return s == 0.0f || (s >= kDnSigmaMin && s <= kDnSigmaMax); } // (NaN fails both)
PM_HD int dn_check(uint32_t iterations, uint32_t normal_power_log2, float sigma_depth, float sigma_luminance) {
	if (iterations > kDnMaxIterations || normal_power_log2 > kDnMaxNormalPowerLog2) return 1;
	if (!dn_sigma_ok(sigma_depth) || !dn_sigma_ok(sigma_luminance)) return 1;
	return 0;
}

} // namespace pol
