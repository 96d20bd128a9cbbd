// temporal.h -- per-pixel arithmetic of the temporal reprojection that polaris_hip_sync_framebuffer runs when temporal reuse is
// on (include/polaris_hip.h, polaris_hip_set_temporal).
//
// ONE definition for both sides, as denoise.h: the HIP kernels (kernels.h, k_reproject / k_temporal; k_gbuffer's centre ray) and
// the CPU restatement the tests compare them with (polaris_amd/host/temporal.cpp) include this header, and both are compiled
// without FMA contraction and with IEEE division and square root, so the two agree bit for bit.  Plain floats only.
//
// The HISTORY is a frame-sized float4 plane (mean rgb | sample count) with the GUIDE / ALBEDO planes and the camera it was seen
// with.  For a filtered pixel i of the current G-buffer the first hit p = eye + t_i d_i is projected into the history camera, and
// the 2 x 2 history pixels around it that saw the same surface give the PRIOR (h rgb | m, m = 0: no history).  The TEMPORAL plane
// then blends the running mean with it: (acc + m h) / (n + m).
// With the option "object_motion"  the history also carries an INSTANCE plane and the instance table it was seen
// with, and p is first taken to where its instance stood then (tp_motion_matrix on the host, tp_reproject<*, true>).
// With the option "vertex_motion"  the history also carries the vertices it was seen with, and the first hit of a
// triangle that a deformation changed is taken to where its barycentric point lay then (tp_reproject<*, true, true>).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "denoise.h"
#include "polaris_math.h"

namespace pol {

constexpr uint32_t kTpMaxHistory = 4096;   // max_history: 0 (off) .. this
constexpr float kTpMaxDepthThreshold = 1e6f;
constexpr float kTpSkew = 1e-3f;           // |tl + br - tr - bl| <= kTpSkew * |tr - tl|: the corners are a parallelogram

// A camera as CameraData carries it: the four frustum corner directions (eye-relative, w = 0) and the eye.
struct TpCamera { float tl[4], tr[4], bl[4], br[4], eye[3]; };

// The unit direction through pixel (gx, gy)'s centre, texel = (1 / W, 1 / H): k_generate's bilinear corner blend with the
// sub-pixel offset fixed at 0.5, over all four components.  k_gbuffer casts this ray, k_reproject re-derives it.
PM_HD void tp_centre_ray(const float tl[4], const float tr[4], const float bl[4], const float br[4], uint32_t gx, uint32_t gy,
                         float texel_x, float texel_y, float d[3]) {
	const float tx = ((float)gx + 0.5f) * texel_x;
	const float ty = ((float)gy + 0.5f) * texel_y;
	const float lx = pm_mix(tl[0], bl[0], ty), ly = pm_mix(tl[1], bl[1], ty), lz = pm_mix(tl[2], bl[2], ty), lw = pm_mix(tl[3], bl[3], ty);
	const float rx = pm_mix(tr[0], br[0], ty), ry = pm_mix(tr[1], br[1], ty), rz = pm_mix(tr[2], br[2], ty), rw = pm_mix(tr[3], br[3], ty);
	const float dx = pm_mix(lx, rx, tx), dy = pm_mix(ly, ry, tx), dz = pm_mix(lz, rz, tx), dw = pm_mix(lw, rw, tx);
	const float inv = 1.0f / pm_sqrt(dx * dx + dy * dy + dz * dz + dw * dw);
	d[0] = dx * inv;
	d[1] = dy * inv;
	d[2] = dz * inv;
}

PM_HD float tp_len3(float x, float y, float z) { return pm_sqrt(x * x + y * y + z * z); }

// A camera is projectable when its corners are a parallelogram (then the bilinear blend of tp_centre_ray is the plane
// tl + u (tr - tl) + v (bl - tl)): every w is 0 and |tl + br - tr - bl| <= kTpSkew |tr - tl|.  A history camera that is not
// gives no history anywhere.
PM_HD bool tp_projectable(const TpCamera &c) {
	if (c.tl[3] != 0.0f || c.tr[3] != 0.0f || c.bl[3] != 0.0f || c.br[3] != 0.0f) return false;
	const float sx = ((c.tl[0] + c.br[0]) - c.tr[0]) - c.bl[0], sy = ((c.tl[1] + c.br[1]) - c.tr[1]) - c.bl[1],
	            sz = ((c.tl[2] + c.br[2]) - c.tr[2]) - c.bl[2];
	return tp_len3(sx, sy, sz) <= kTpSkew * tp_len3(c.tr[0] - c.tl[0], c.tr[1] - c.tl[1], c.tr[2] - c.tl[2]); // (NaN fails)
}

// det(a, b, c) = a . (b x c), in this order
PM_HD float tp_det(const float a[3], const float b[3], const float c[3]) {
	return a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// Projection of the point p into camera c (projectable): solves tl + u A + v B = mu q, A = tr - tl, B = bl - tl, q = p - eye, by
// Cramer's rule: D = det(A, B, q), u = -det(tl, B, q) / D, v = -det(A, tl, q) / D, mu = det(A, B, tl) / D.  Returns false unless
// mu > 0 (the point lies in front of the camera; D = 0 or a NaN fails too).  dist = |q|.
PM_HD bool tp_project(const TpCamera &c, const float p[3], float &u, float &v, float &dist) {
	const float A[3] = {c.tr[0] - c.tl[0], c.tr[1] - c.tl[1], c.tr[2] - c.tl[2]};
	const float B[3] = {c.bl[0] - c.tl[0], c.bl[1] - c.tl[1], c.bl[2] - c.tl[2]};
	const float q[3] = {p[0] - c.eye[0], p[1] - c.eye[1], p[2] - c.eye[2]};
	const float T[3] = {c.tl[0], c.tl[1], c.tl[2]};
	const float D = tp_det(A, B, q);
	const float mu = tp_det(A, B, T) / D;
	if (!(mu > 0.0f)) return false;
	u = -tp_det(T, B, q) / D;
	v = -tp_det(A, T, q) / D;
	dist = tp_len3(q[0], q[1], q[2]);
	return true;
}

// ---- polaris_hip_set_projection: the orthographic and the equirectangular camera.  The view basis and the two extents of
// the kind in force (ORTHOGRAPHIC: half_width, half_height; EQUIRECTANGULAR: lon_range, lat_range) with the eye.  The history camera and
// the current one always share one projection (a changed projection drops the history): they differ in the eye alone.
constexpr uint32_t kTpOrthographic = 1, kTpEquirectangular = 2; // POLARIS_PROJECTION_*
struct TpProjection { uint32_t kind; float axis[3], right[3], up[3], ex, ey; };
struct TpProjCamera { TpProjection proj; float eye[3]; };

// The ray of a projected camera at the frame coordinates (tx, ty) in [0, 1): k_generate_proj's lines after tx and ty, every operation
// rounded once in the order written.  ORTHOGRAPHIC: the origin moves in the window, the direction is the axis verbatim.
// EQUIRECTANGULAR: the origin is the eye, the direction the unit vector at longitude (tx - 0.5) lon_range, latitude (0.5 - ty) lat_range.
// KIND is the projection's kind, which k_generate_proj<KIND> knows as it is compiled; tp_proj_ray reads it from P.
// (The ray is returned by value and the two kinds' results meet as values: written through o[] and d[] inside the branch, the device
// compiler keeps the arrays in scratch memory.)
struct TpRay { float ox, oy, oz, dx, dy, dz; };
template <uint32_t KIND>
PM_HD TpRay tp_proj_ray_of(const TpProjection &P, const float eye[3], float tx, float ty) {
	if constexpr (KIND == kTpOrthographic) {
		const float sx = 2.0f * tx - 1.0f, sy = 1.0f - 2.0f * ty;
		const float a = sx * P.ex, b = sy * P.ey;
		return TpRay{(eye[0] + P.right[0] * a) + P.up[0] * b, (eye[1] + P.right[1] * a) + P.up[1] * b, (eye[2] + P.right[2] * a) + P.up[2] * b,
		             P.axis[0], P.axis[1], P.axis[2]};
	} else {
		const float lon = (tx - 0.5f) * P.ex, lat = (0.5f - ty) * P.ey;
		const float cl = pm_cos(lat), sl = pm_sin(lat), co = pm_cos(lon), so = pm_sin(lon);
		const float a = cl * co, b = cl * so;
		const float ex = (P.axis[0] * a + P.right[0] * b) + P.up[0] * sl;
		const float ey = (P.axis[1] * a + P.right[1] * b) + P.up[1] * sl;
		const float ez = (P.axis[2] * a + P.right[2] * b) + P.up[2] * sl;
		const float inv = 1.0f / pm_sqrt((ex * ex + ey * ey) + ez * ez);
		return TpRay{eye[0], eye[1], eye[2], ex * inv, ey * inv, ez * inv};
	}
}
PM_HD void tp_proj_ray(const TpProjection &P, const float eye[3], float tx, float ty, float o[3], float d[3]) {
	const TpRay r = P.kind == kTpOrthographic ? tp_proj_ray_of<kTpOrthographic>(P, eye, tx, ty) : tp_proj_ray_of<kTpEquirectangular>(P, eye, tx, ty);
	o[0] = r.ox; o[1] = r.oy; o[2] = r.oz;
	d[0] = r.dx; d[1] = r.dy; d[2] = r.dz;
}

// The guide ray of pixel (gx, gy): the ray through the pixel's centre, which the G-buffer kernels cast and the reprojection re-derives.
// The perspective camera's starts at the eye along tp_centre_ray; a projected camera's is tp_proj_ray with the offset fixed at 0.5.
PM_HD void tp_guide_ray(const TpCamera &c, uint32_t gx, uint32_t gy, float texel_x, float texel_y, float o[3], float d[3]) {
	tp_centre_ray(c.tl, c.tr, c.bl, c.br, gx, gy, texel_x, texel_y, d);
	o[0] = c.eye[0]; o[1] = c.eye[1]; o[2] = c.eye[2];
}
PM_HD void tp_guide_ray(const TpProjCamera &c, uint32_t gx, uint32_t gy, float texel_x, float texel_y, float o[3], float d[3]) {
	tp_proj_ray(c.proj, c.eye, ((float)gx + 0.5f) * texel_x, ((float)gy + 0.5f) * texel_y, o, d);
}

// tp_project for a projected camera: q = p - eye in the view basis, x = q . axis, y = q . right, z = q . up, each dot summed left to
// right.  ORTHOGRAPHIC: fails unless x > 0; dist = x, the distance along the axis, which is what GUIDE t holds under it.
// EQUIRECTANGULAR: dist = |q|, fails unless dist > 0 (NaN fails).  No wrap across the seam: a point outside the frame gets a (u, v)
// outside [0, 1] and falls under tp_reproject's bounds rule.
PM_HD bool tp_project(const TpProjCamera &c, const float p[3], float &u, float &v, float &dist) {
	const TpProjection &P = c.proj;
	const float q[3] = {p[0] - c.eye[0], p[1] - c.eye[1], p[2] - c.eye[2]};
	const float x = (q[0] * P.axis[0] + q[1] * P.axis[1]) + q[2] * P.axis[2];
	const float y = (q[0] * P.right[0] + q[1] * P.right[1]) + q[2] * P.right[2];
	const float z = (q[0] * P.up[0] + q[1] * P.up[1]) + q[2] * P.up[2];
	if (P.kind == kTpOrthographic) {
		if (!(x > 0.0f)) return false;
		u = (y / P.ex + 1.0f) * 0.5f;
		v = (1.0f - z / P.ey) * 0.5f;
		dist = x;
		return true;
	}
	dist = tp_len3(q[0], q[1], q[2]);
	if (!(dist > 0.0f)) return false;
	const float lon = pm_atan2(y, x), lat = pm_atan2(z, pm_sqrt(x * x + y * y));
	u = lon / P.ex + 0.5f;
	v = 0.5f - lat / P.ey;
	return true;
}
PM_HD bool tp_projectable(const TpProjCamera &) { return true; } // (polaris_hip_set_projection checked the basis and the extents)

// One history tap as k_reproject gathers it (m2: the history's M2, gathered only by k_reproject<true, *>, variance.h; inst: the
// history's INSTANCE word, gathered only by k_reproject<*, true>).
struct TpTap { float r, g, b, count; float nx, ny, nz, t; float leaf; float m2; uint32_t inst; };

// Object motion (option "object_motion"): what became of mesh instance k between the history and now, one entry of
// the motion table per instance.  STATIC: the instance has not moved, p as without the option.  MOVED: a first hit p of the
// current frame lay at D p when the history was seen (D the affine 3 x 4, rows r0, r1, r2).  INVALID: no history for its pixels.
enum : uint32_t { kTpStatic = 0, kTpMoved = 1, kTpInvalid = 2 };
constexpr uint32_t kTpNoInstance = 0xFFFFFFFFu; // the INSTANCE word of a miss
constexpr uint32_t kTpMaxInstances = 1u << 20;   // of polaris_hip_reproject_motion_planes / polaris_host_reproject_motion
struct TpNoMotion {}; // (tp_reproject<*, false> never calls its motion argument)
constexpr uint32_t kTpNoTriangle = 0xFFFFFFFFu; // the HIT plane's triangle word of a miss (option "vertex_motion")
constexpr uint32_t kTpMaxTriangles = 1u << 24;   // of polaris_hip_reproject_deform_planes / polaris_host_reproject_deform
struct TpNoDeform {}; // (tp_reproject<*, *, false> never calls its two deformation arguments)

// ---- host only (plain functions: no device code is generated for them) ----
// The camera of an eye and the sixteen floats of its frustum corners (tl, tr, bl, br), as CameraData and the test entries carry them.
inline TpCamera tp_camera(const float eye[3], const float fr[16]) {
	return TpCamera{{fr[0], fr[1], fr[2], fr[3]}, {fr[4], fr[5], fr[6], fr[7]}, {fr[8], fr[9], fr[10], fr[11]}, {fr[12], fr[13], fr[14], fr[15]},
	                {eye[0], eye[1], eye[2]}};
}

// The motion table's entry of one instance from its two inv_transform (PolarisMeshInstance: column major, world -> mesh; the
// affine rows 0-2 are what the traversal uses): STATIC when the two are byte-equal, else D = inverse(Inv_hist) . Inv_cur in double
// precision (cofactor inversion of the upper 3 x 3), rounded to float once at the end.  INVALID when either upper 3 x 3 has a
// determinant of 0 or a non-finite one, or an entry of D is not finite after rounding.  D is the identity for STATIC, 0 for INVALID.
// Host only: the library (where the PRIOR is computed) and the CPU restatement both call it.
inline uint32_t tp_motion_matrix(const float inv_hist[16], const float inv_cur[16], float D[12]) {
	for (int k = 0; k < 12; k++) D[k] = 0.0f;
	if (memcmp(inv_hist, inv_cur, 16 * sizeof(float)) == 0) {
		D[0] = D[5] = D[10] = 1.0f;
		return kTpStatic;
	}
	double a[3][3], c[3][3], dt[3];
	for (int r = 0; r < 3; r++) {
		for (int k = 0; k < 3; k++) { a[r][k] = (double)inv_hist[4 * k + r]; c[r][k] = (double)inv_cur[4 * k + r]; }
		dt[r] = (double)inv_cur[12 + r] - (double)inv_hist[12 + r];
	}
	auto det3 = [](const double m[3][3], double co[3]) {
		co[0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
		co[1] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
		co[2] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
		return m[0][0] * co[0] + m[0][1] * co[1] + m[0][2] * co[2];
	};
	double co[3], cc[3];
	const double det = det3(a, co), det_cur = det3(c, cc);
	if (!(det != 0.0) || !isfinite(det) || !(det_cur != 0.0) || !isfinite(det_cur)) return kTpInvalid;
	const double inv[3][3] = {
		{co[0] / det, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det},
		{co[1] / det, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det},
		{co[2] / det, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det}};
	bool finite = true;
	for (int r = 0; r < 3; r++) {
		for (int k = 0; k < 3; k++) D[4 * r + k] = (float)((inv[r][0] * c[0][k] + inv[r][1] * c[1][k]) + inv[r][2] * c[2][k]);
		D[4 * r + 3] = (float)((inv[r][0] * dt[0] + inv[r][1] * dt[1]) + inv[r][2] * dt[2]);
		for (int k = 0; k < 4; k++) finite = finite && isfinite(D[4 * r + k]);
	}
	if (!finite) {
		for (int k = 0; k < 12; k++) D[k] = 0.0f;
		return kTpInvalid;
	}
	return kTpMoved;
}

// The motion table as it is uploaded, four float4 per instance: rows r0, r1, r2 of D, then the flag word (bits of .x) | 0 | 0 | 0.
inline void tp_motion_table(uint32_t n_instances, const float *inv_hist, const float *inv_cur, float *table) {
	for (uint32_t k = 0; k < n_instances; k++) {
		float *e = table + 16 * (size_t)k;
		const uint32_t flag = tp_motion_matrix(inv_hist + 16 * (size_t)k, inv_cur + 16 * (size_t)k, e);
		memcpy(e + 12, &flag, sizeof flag);
		e[13] = e[14] = e[15] = 0.0f;
	}
}

// The deformation table (option "vertex_motion"), beside the motion table and in its layout: per instance M = inverse(Inv_hist), mesh
// space -> the world of the history, which is tp_motion_matrix against the identity.  STATIC: M is the identity.
inline void tp_deform_table(uint32_t n_instances, const float *inv_hist, float *table) {
	const float identity[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
	for (uint32_t k = 0; k < n_instances; k++) {
		float *e = table + 16 * (size_t)k;
		const uint32_t flag = tp_motion_matrix(inv_hist + 16 * (size_t)k, identity, e);
		memcpy(e + 12, &flag, sizeof flag);
		e[13] = e[14] = e[15] = 0.0f;
	}
}

// The tap test: a history count > 0, finite history rgb, the same leaf word as pixel i, n_i . n_j >= normal_threshold and
// |t_j - dist| <= depth_threshold * dist.
PM_HD bool tp_finite(float x) { return (pm_f2u(x) & 0x7f800000u) != 0x7f800000u; }
PM_HD bool tp_tap_ok(const TpTap &j, float leaf_i, float nx, float ny, float nz, float dist, float normal_threshold, float depth_threshold) {
	if (!(j.count > 0.0f)) return false;
	if (!tp_finite(j.r) || !tp_finite(j.g) || !tp_finite(j.b)) return false;
	if (pm_f2u(j.leaf) != pm_f2u(leaf_i)) return false;
	if (!(nx * j.nx + ny * j.ny + nz * j.nz >= normal_threshold)) return false;
	return pm_fabs(j.t - dist) <= depth_threshold * dist;
}

// The PRIOR of pixel (gx, gy) of a W x H frame: guide_i / leaf_i of the current G-buffer, cur / hist the cameras (hist
// projectable), load(j, tap) fills history tap j (row-major index).  out = h rgb | m; m = 0 (and h = 0) without history.
// The taps are the 2 x 2 around (u W - 0.5, v H - 0.5) in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1);
// their bilinear weights are renormalised over the valid ones.  M2 (variance guidance with temporal reuse): the taps' m2 are
// blended with the same weights into out2 = h2 | 0 | 0 | m (all 0 without history); M2 = false leaves out2 alone.
// MOTION (option "object_motion"): inst_i is the pixel's INSTANCE word and motion(k, D) gives instance k's motion table entry, the
// flag returned and, for MOVED, D's twelve floats filled in (k < n_inst; a word outside the table gives no history).  INVALID:
// m = 0.  MOVED: p becomes D p, each row ((r.x px + r.y py) + r.z pz) + r.w, before the projection, so the depth test sees
// |D p - eye'|.  A tap must also carry the INSTANCE word inst_i.  MOTION = false reads neither.
// DEFORM (option "vertex_motion", with MOTION): hit_i is the pixel's HIT word (scene triangle T | bits of u | bits of v) and
// verts(T, a, b) fills the xyz of T's three vertices, a as the scene holds them now and b as the history saw them (T < n_tris; a
// word outside gives no history).  36 equal bytes: the pixel takes MOTION's path, unchanged.  Else p becomes M q, q the point of
// the old triangle at the hit's barycentrics (surface_at's expression) and matrix(k, M) instance k's deformation table entry
// (tp_deform_table: STATIC p = q, INVALID m = 0, MOVED the rows as D's); a component of q or p that is not finite: m = 0.
// DEFORM = false reads none of it.
// Camera: TpCamera, or TpProjCamera under polaris_hip_set_projection (cur and hist of one projection): tp_guide_ray and tp_project are
// the camera's, everything else is the same.
template <bool M2 = false, bool MOTION = false, bool DEFORM = false, class Load, class Motion = TpNoMotion, class Verts = TpNoDeform,
          class Matrix = TpNoDeform, class Camera = TpCamera>
PM_HD void tp_reproject(uint32_t gx, uint32_t gy, uint32_t W, uint32_t H, const float guide_i[4], float leaf_i, const Camera &cur,
                        const Camera &hist, uint32_t max_history, float normal_threshold, float depth_threshold, Load load, float out[4],
                        float *out2 = nullptr, uint32_t inst_i = 0, uint32_t n_inst = 0, Motion motion = Motion(),
                        const uint32_t *hit_i = nullptr, uint32_t n_tris = 0, Verts verts = Verts(), Matrix matrix = Matrix()) {
	static_assert(MOTION || !DEFORM, "DEFORM extends MOTION");
	out[0] = out[1] = out[2] = out[3] = 0.0f;
	if (M2) out2[0] = out2[1] = out2[2] = out2[3] = 0.0f;
	if (!dn_filtered(leaf_i)) return;
	float o[3], d[3];
	tp_guide_ray(cur, gx, gy, 1.0f / (float)W, 1.0f / (float)H, o, d);
	const float t = guide_i[3];
	float p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
	bool rigid = true; // (the pixel's triangle is as the history saw it)
	if constexpr (DEFORM) {
		if (inst_i >= n_inst || hit_i[0] >= n_tris) return;
		float a[9], b[9];
		verts(hit_i[0], a, b);
		for (int k = 0; k < 9; k++) rigid = rigid && pm_f2u(a[k]) == pm_f2u(b[k]);
		if (!rigid) {
			const float bu = pm_u2f(hit_i[1]), bv = pm_u2f(hit_i[2]);
			const float bw = 1.0f - (bu + bv);
			const float qx = bw * b[0] + bu * b[3] + bv * b[6], qy = bw * b[1] + bu * b[4] + bv * b[7], qz = bw * b[2] + bu * b[5] + bv * b[8];
			if (!tp_finite(qx) || !tp_finite(qy) || !tp_finite(qz)) return;
			float M[12];
			const uint32_t flag = matrix(inst_i, M);
			if (flag == kTpMoved) {
				p[0] = ((M[0] * qx + M[1] * qy) + M[2] * qz) + M[3];
				p[1] = ((M[4] * qx + M[5] * qy) + M[6] * qz) + M[7];
				p[2] = ((M[8] * qx + M[9] * qy) + M[10] * qz) + M[11];
			} else if (flag == kTpStatic) {
				p[0] = qx; p[1] = qy; p[2] = qz;
			} else return;
			if (!tp_finite(p[0]) || !tp_finite(p[1]) || !tp_finite(p[2])) return;
		}
	}
	if constexpr (MOTION) {
		if (inst_i >= n_inst) return;
		if (rigid) {
			float D[12];
			const uint32_t flag = motion(inst_i, D);
			if (flag == kTpMoved) {
				const float px = p[0], py = p[1], pz = p[2];
				p[0] = ((D[0] * px + D[1] * py) + D[2] * pz) + D[3];
				p[1] = ((D[4] * px + D[5] * py) + D[6] * pz) + D[7];
				p[2] = ((D[8] * px + D[9] * py) + D[10] * pz) + D[11];
			} else if (flag != kTpStatic) return;
		}
	}
	float u, v, dist;
	if (!tp_project(hist, p, u, v, dist)) return;
	const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
	if (!(x > -1.0f && x < (float)W && y > -1.0f && y < (float)H)) return; // (no tap inside; NaN fails)
	const float fx0 = pm_floor(x), fy0 = pm_floor(y);
	const float fx = x - fx0, fy = y - fy0;
	const int x0 = (int)fx0, y0 = (int)fy0;
	float sw = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hc = 0.0f, h2 = 0.0f;
	for (int k = 0; k < 4; k++) {
		const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
		if (xx < 0 || xx >= (int)W || yy < 0 || yy >= (int)H) continue;
		const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
		TpTap j;
		load((uint32_t)yy * W + (uint32_t)xx, j);
		if (MOTION && j.inst != inst_i) continue;
		if (!tp_tap_ok(j, leaf_i, guide_i[0], guide_i[1], guide_i[2], dist, normal_threshold, depth_threshold)) continue;
		sw += w;
		hr += w * j.r;
		hg += w * j.g;
		hb += w * j.b;
		hc += w * j.count;
		if (M2) h2 += w * j.m2;
	}
	if (!(sw > 0.0f)) return;
	const float m = pm_min(hc / sw, (float)max_history);
	if (!(m > 0.0f)) return;
	out[0] = hr / sw;
	out[1] = hg / sw;
	out[2] = hb / sw;
	out[3] = m;
	if (M2) {
		out2[0] = h2 / sw;
		out2[3] = m;
	}
}

// The TEMPORAL pixel from the frame accumulator's a[4], the PRIOR's pr[4], n = accumulated_samples + samples_per_pixel as a float
// and sync's weight 1 / n: m > 0 -> (a + m h) / (n + m) | n + m; m = 0 -> a * weight | n, the running mean sync tone-maps today.
PM_HD void tp_combine(const float a[4], const float pr[4], float n, float weight, float out[4]) {
	const float m = pr[3];
	if (m > 0.0f) {
		const float s = n + m;
		out[0] = (a[0] + m * pr[0]) / s;
		out[1] = (a[1] + m * pr[1]) / s;
		out[2] = (a[2] + m * pr[2]) / s;
		out[3] = s;
	} else {
		out[0] = a[0] * weight;
		out[1] = a[1] * weight;
		out[2] = a[2] * weight;
		out[3] = n;
	}
}

// Parameter check shared by polaris_hip_set_temporal, polaris_hip_reproject_planes and polaris_host_reproject: 0 = valid.
PM_HD int tp_check(uint32_t max_history, float normal_threshold, float depth_threshold) {
	if (max_history > kTpMaxHistory) return 1;
	if (!(normal_threshold >= -1.0f && normal_threshold <= 1.0f)) return 1;       // (NaN fails)
	if (!(depth_threshold >= 0.0f && depth_threshold <= kTpMaxDepthThreshold)) return 1;
	return 0;
}

} // namespace pol
