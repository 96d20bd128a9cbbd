// variance.h -- per-pixel arithmetic of the variance estimate and the variance-guided a-trous filter (Schied et al. 2017, SVGF)
// that polaris_hip_sync_framebuffer runs when variance guidance is on (include/polaris_hip.h, polaris_hip_set_variance; DESIGN.md
// 10c), and the luminance whose square the batch epilogue accumulates when the tracer option "moments" is on.
//
// ONE definition for both sides, as denoise.h / temporal.h: the HIP kernels (kernels.h, k_resolve<true> / k_aggregate<true>,
// k_variance, k_denoise_variance) and the CPU restatement the tests compare them with (polaris_amd/host/variance.cpp) include this
// header, and both are compiled without FMA contraction and with IEEE division and square root, so the two agree bit for bit.
//
// Moments: with "moments" on, a frame accumulator pixel is rgb = sum of the samples' radiance | w = sum of L_s^2, L_s = va_lum of
// sample s.  The VARIANCE plane holds M1 | M2 | n_eff | v per pixel: the luminance of the synced mean, the mean of L^2, the
// effective sample count and the variance of the mean.
#pragma once

#include <stdint.h>

#include "denoise.h"
#include "polaris_math.h"

namespace pol {

constexpr float kVaEps = 1e-10f;              // the guided luminance term's denominator floor: sigma_v sqrt(g(v)) + kVaEps
constexpr uint32_t kVaMaxMinSamples = 64;     // min_samples: 1 .. this
constexpr int kVaRadius = 3;                  // the spatial fallback's window: (2 kVaRadius + 1)^2 at stride 1

// Rec. 709 luminance, (0.2126 r + 0.7152 g) + 0.0722 b in this order (no contraction on either side).
PM_HD float va_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
PM_HD float va_lum2(float r, float g, float b) {
	const float l = va_lum(r, g, b);
	return l * l;
}

// The moments of one pixel: c = the synced mean (acc rgb * weight, or the TEMPORAL plane's rgb), a_w = the frame accumulator's
// sum of L^2, n = accumulated_samples + samples_per_pixel as a float, weight = sync's 1 / n, and the history's M2 h2 with its
// count m (m = 0: none).  out = M1 | M2 | n_eff: M2 = (a_w + m h2) / (n + m) where m > 0 (tp_combine's form), a_w * weight otherwise.
PM_HD void va_moments(const float c[3], float a_w, float n, float weight, float m, float h2, float out[3]) {
	out[0] = va_lum(c[0], c[1], c[2]);
	if (m > 0.0f) {
		const float s = n + m;
		out[1] = (a_w + m * h2) / s;
		out[2] = s;
	} else {
		out[1] = a_w * weight;
		out[2] = n;
	}
}

// The variance of the mean of the filtered pixel (x, y) with moments mi (M1 | M2 | n_eff) and guide ci (normal | distance):
//   n_eff >= max(min_samples, 2): max(0, M2 - M1^2) / (n_eff - 1);
//   otherwise the spatial fallback over the 7 x 7 taps at stride 1 (dy outer, dx inner) inside the rows [y0, y1) and the frame
//   width that are filtered, weighted by dn_weight(1, ...) of `it` (step 1, luminance term off: w_n w_z; the centre weighs 1):
//   s^2 = max(0, sum w M2 / sum w - (sum w M1 / sum w)^2), v = s^2 / n_eff.
// load(j, tap, m) fills tap j's guide (tap.r/g/b unused) and its moments m[3], and returns whether it is filtered.
template <class Load>
PM_HD float va_estimate(uint32_t x, uint32_t y, uint32_t W, uint32_t y0, uint32_t y1, const DnTap &ci, const float mi[3], uint32_t min_samples,
                        const DnIter &it, Load load) {
	const float ne = mi[2];
	if (ne >= (float)min_samples && ne >= 2.0f) return pm_max(0.0f, mi[1] - mi[0] * mi[0]) / (ne - 1.0f);
	float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
	for (int dy = -kVaRadius; dy <= kVaRadius; dy++) {
		const int yy = (int)y + dy;
		if (yy < (int)y0 || yy >= (int)y1) continue;
		for (int dx = -kVaRadius; dx <= kVaRadius; dx++) {
			const int xx = (int)x + dx;
			if (xx < 0 || xx >= (int)W) continue;
			float w, mj[3];
			if (dx == 0 && dy == 0) {
				w = 1.0f;
				mj[0] = mi[0]; mj[1] = mi[1];
			} else {
				DnTap cj;
				if (!load((uint32_t)yy * W + (uint32_t)xx, cj, mj)) continue;
				w = dn_weight(1.0f, ci, cj, it);
			}
			sw += w;
			s1 += w * mj[0];
			s2 += w * mj[1];
		}
	}
	const float m1 = s1 / sw, m2 = s2 / sw;
	return pm_max(0.0f, m2 - m1 * m1) / ne;
}

// Iteration 0's variance of the demodulated radiance: v / lum(a')^2, a' = the per-channel demodulation albedo (exact for grey albedo).
PM_HD float va_demod(float v, const float a[3]) { return v / va_lum2(dn_demod_albedo(a[0]), dn_demod_albedo(a[1]), dn_demod_albedo(a[2])); }
PM_HD float va_remod(float v, const float a[3]) { return v * va_lum2(dn_demod_albedo(a[0]), dn_demod_albedo(a[1]), dn_demod_albedo(a[2])); }

// {1/4, 1/2, 1/4} taps, index 0..2
PM_HD float va_g(int i) { return i == 1 ? 0.5f : 0.25f; }

// One variance-guided a-trous iteration for the filtered pixel (x, y): dn_step's 5 x 5 taps at stride s, skip rules and centre
// weight, with the luminance term of `it` replaced by w_l = exp(-|lum(r_i) - lum(r_j)| / (sigma_v sqrt(g(v_i)) + kVaEps)), where
// g(v_i) = sum h v_j / sum h over the 3 x 3 taps at stride 1 (h = {1/4, 1/2, 1/4}^2; dy outer, dx inner; filtered taps inside the
// rows and the width).  w_j = dn_weight(h, ...) (it.lum_scale = 0) * w_l.  out = sum w r / sum w | sum w^2 v / (sum w)^2.
// load(j, tap, v) fills tap j (demodulated radiance r^k) and its variance v^k, and returns whether it is filtered.
template <class Load>
PM_HD void va_step(uint32_t x, uint32_t y, uint32_t W, uint32_t y0, uint32_t y1, const DnTap &ci, float vi, const DnIter &it, float sigma_v,
                   Load load, float out[4]) {
	float gh = 0.0f, gv = 0.0f;
	for (int dy = -1; dy <= 1; dy++) {
		const int yy = (int)y + dy;
		if (yy < (int)y0 || yy >= (int)y1) continue;
		for (int dx = -1; dx <= 1; dx++) {
			const int xx = (int)x + dx;
			if (xx < 0 || xx >= (int)W) continue;
			const float h = va_g(dx + 1) * va_g(dy + 1);
			float vj = vi;
			if (dx != 0 || dy != 0) {
				DnTap cj;
				if (!load((uint32_t)yy * W + (uint32_t)xx, cj, vj)) continue;
			}
			gh += h;
			gv += h * vj;
		}
	}
	const float denom = sigma_v * pm_sqrt(gv / gh) + kVaEps;
	const float li = va_lum(ci.r, ci.g, ci.b);
	float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, sv = 0.0f;
	const int s = (int)it.step;
	for (int dy = -2; dy <= 2; dy++) {
		const int yy = (int)y + dy * s;
		if (yy < (int)y0 || yy >= (int)y1) continue;
		for (int dx = -2; dx <= 2; dx++) {
			const int xx = (int)x + dx * s;
			if (xx < 0 || xx >= (int)W) continue;
			const float h = dn_h(dx + 2) * dn_h(dy + 2);
			float w, vj;
			DnTap cj;
			if (dx == 0 && dy == 0) {
				w = h;
				cj = ci;
				vj = vi;
			} else {
				if (!load((uint32_t)yy * W + (uint32_t)xx, cj, vj)) continue;
				w = dn_weight(h, ci, cj, it) * pm_exp(-pm_fabs(li - va_lum(cj.r, cj.g, cj.b)) / denom);
			}
			sw += w;
			ar += w * cj.r;
			ag += w * cj.g;
			ab += w * cj.b;
			sv += (w * w) * vj;
		}
	}
	out[0] = ar / sw;
	out[1] = ag / sw;
	out[2] = ab / sw;
	out[3] = sv / (sw * sw);
}

// Parameter check shared by polaris_hip_set_variance, polaris_hip_variance_planes and the host restatement: 0 = valid.  sigma_v = 0
// is off (min_samples is then not looked at); on, sigma_v within [1e-6, 1e6] and min_samples within 1..64.
PM_HD int va_check(float sigma_variance, uint32_t min_samples) {
	if (!dn_sigma_ok(sigma_variance)) return 1;
	if (sigma_variance != 0.0f && (min_samples < 1 || min_samples > kVaMaxMinSamples)) return 1;
	return 0;
}

} // namespace pol
