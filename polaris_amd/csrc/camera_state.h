// camera_state.h -- the camera of a tracer handle as the caller sent it, as pure host code: the open camera (polaris_hip_set_camera),
// the lens (polaris_hip_set_lens) and the close state of the shutter (polaris_hip_set_shutter), which of the four ray generators they
// ask for, the projection (polaris_hip_set_projection), and the rules that tie the setters together, one named transition per setter:
//   - a new camera switches the shutter off (the close state belonged to the camera that goes);
//   - a changed lens switches the shutter off and drops the temporal history; identical bytes do nothing;
//   - a shutter needs a camera; its close lens is checked only while the lens is on; identical bytes, or off and off, do nothing;
//   - a projection needs a camera and excludes the lens and the shutter, in both directions; a changed projection drops the G-buffer
//     and the temporal history; identical bytes, or off and off, do nothing; a new camera keeps it;
//   - a refusal changes nothing.
// A transition does not change the state it is asked on: it returns the refusal, or what the owner must do and the state to commit
// once that is done, so a step of the owner's that fails leaves the camera as it was.
//
// No HIP here and no device pointer: polaris_hip.hip builds the kernels' arguments from this state (camera_args) and performs what a
// transition returns; tests/tools/camera_state_check.cpp asks the same functions on a CPU.  DESIGN.md sections 10h, 10j and 10n describe the features.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "polaris_hip.h"

namespace pol {

static_assert(sizeof(PolarisLensParams) == 44 && offsetof(PolarisLensParams, focus_distance) == 4, "PolarisLensParams is struct_size and ten floats");
static_assert(sizeof(PolarisShutterParams) == 124 && offsetof(PolarisShutterParams, eye1) == 8 && offsetof(PolarisShutterParams, focus_distance1) == 84,
              "PolarisShutterParams is struct_size, enabled, 19 camera floats and ten lens floats");
static_assert(sizeof(PolarisProjectionParams) == 60 && offsetof(PolarisProjectionParams, axis) == 8 && offsetof(PolarisProjectionParams, half_width) == 44 &&
              offsetof(PolarisProjectionParams, lat_range) == 56, "PolarisProjectionParams is struct_size, kind and 13 floats");

struct CameraFloats { float eye[3], frustum[16]; }; // polaris_hip_set_camera's arguments (frustum: the corner rays TL, TR, BL, BR)

// k_generate, k_generate_lens, k_generate_shutter<false>, k_generate_shutter<true>, k_generate_proj<1>, k_generate_proj<2>
enum class Generator { Pinhole, Lens, Shutter, ShutterLens, Ortho, Equirect };

// What the owner does for a transition, in this order, before it commits the state (a set of bits).
enum CameraTodo : uint32_t {
	kCamDropHistory = 1, // the temporal history saw another lens or shutter: the main stream idle, then FrameSync::lens_changed
	kCamMoved = 2,       // FrameSync::camera_moved with the camera that goes
	kCamShutterOff = 4,  // the shutter goes from on to off (nothing to do beyond kCamDropHistory, which comes with it: the committed state has it off)
	kCamProjection = 8,  // the G-buffer and the history were seen through another projection: the main stream idle, then FrameSync::projection_changed
};

inline std::string camera_words(const char *fmt, ...) { // a refusal's words
	char buf[256];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	return buf;
}
// The rules for the ten floats of a lens (focus distance, axis, u, v), for polaris_hip_set_lens and the close lens of
// polaris_hip_set_shutter (`who`): all finite, entries of u and v at most 2^30, and for a lens that is `on` the ranges of the focus
// distance and of the axis' length.  Empty, or the refusal.
inline std::string check_lens_floats(const char *who, const float *f, bool on) {
	for (int i = 0; i < 10; i++)
		if (!std::isfinite(f[i])) return camera_words("%s: float %d is not finite", who, i);
	for (int i = 4; i < 10; i++)
		if (std::fabs(f[i]) > 0x1p30f) return camera_words("%s: an entry of u or v is above 2^30", who);
	if (!on) return "";
	if (!(f[0] >= 1e-6f && f[0] <= 1e30f)) return camera_words("%s: focus_distance %g outside [1e-6, 1e30]", who, (double)f[0]);
	const float a2 = f[1] * f[1] + f[2] * f[2] + f[3] * f[3];
	if (!(a2 >= 0.998f && a2 <= 1.002f)) return camera_words("%s: axis is not a unit vector (squared length %g)", who, (double)a2);
	return "";
}

struct CameraStep;
struct CameraState {
	bool have_camera = false;
	CameraFloats open{};
	PolarisLensParams lens{sizeof(PolarisLensParams), 0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}; // u = v = 0: off
	PolarisShutterParams shutter{sizeof(PolarisShutterParams), 0u, {}, {}, 0.0f, {}, {}, {}}; // the camera and lens at shutter close; enabled = 0: off

	PolarisProjectionParams projection{sizeof(PolarisProjectionParams), POLARIS_PROJECTION_PERSPECTIVE, {}, {}, {}, 0.0f, 0.0f, 0.0f, 0.0f}; // kind = 0: off

	bool lens_on() const { for (int i = 0; i < 3; i++) if (lens.u[i] != 0.0f || lens.v[i] != 0.0f) return true; return false; }
	bool shutter_on() const { return shutter.enabled != 0; }
	bool projection_on() const { return projection.kind != POLARIS_PROJECTION_PERSPECTIVE; }
	Generator generator() const {
		if (projection_on()) return projection.kind == POLARIS_PROJECTION_ORTHOGRAPHIC ? Generator::Ortho : Generator::Equirect; // (neither lens nor shutter is on)
		return generator_of_frustum();
	}
	Generator generator_of_frustum() const { return shutter_on() ? (lens_on() ? Generator::ShutterLens : Generator::Shutter) : (lens_on() ? Generator::Lens : Generator::Pinhole); }

	// ---- the transitions (all refusals are POLARIS_E_BAD_ARGUMENT)
	inline CameraStep set_camera(const float *eye, const float *frustum) const;
	inline CameraStep set_lens(const PolarisLensParams *p) const;
	inline CameraStep set_shutter(const PolarisShutterParams *p) const;
	inline CameraStep set_projection(const PolarisProjectionParams *p) const;
};

struct CameraStep {
	std::string refusal; // not empty: refused, in these words; nothing else is set
	uint32_t todo = 0;   // CameraTodo bits; 0 with an empty refusal: nothing happens, `next` is the state as it is
	CameraState next;    // what the owner commits after `todo`
};

inline CameraStep CameraState::set_camera(const float *eye, const float *frustum) const {
	if (!eye || !frustum) return {"camera pointers are null", 0, *this};
	CameraStep s{"", kCamMoved, *this};
	if (shutter_on()) s.todo |= kCamShutterOff | kCamDropHistory;
	s.next.shutter.enabled = 0;
	memcpy(s.next.open.eye, eye, sizeof s.next.open.eye);
	memcpy(s.next.open.frustum, frustum, sizeof s.next.open.frustum);
	s.next.have_camera = true;
	return s;
}

inline CameraStep CameraState::set_lens(const PolarisLensParams *p) const {
	if (!p || p->struct_size != sizeof(PolarisLensParams)) return {camera_words("set_lens: null params or struct_size != %zu", sizeof(PolarisLensParams)), 0, *this};
	const float *f = &p->focus_distance; // the ten floats after struct_size
	bool on = false; // (a NaN in u or v counts as on here and is refused below)
	for (int i = 4; i < 10; i++) on = on || f[i] != 0.0f;
	std::string why = check_lens_floats("set_lens", f, on);
	if (!why.empty()) return {why, 0, *this};
	if (on && projection_on()) return {"set_lens: a lens under a projection other than the perspective one (polaris_hip_set_projection) is not supported", 0, *this};
	if (memcmp(p, &lens, sizeof lens) == 0) return {"", 0, *this}; // identical bytes: nothing happens
	CameraStep s{"", kCamDropHistory | (shutter_on() ? kCamShutterOff : 0u), *this};
	s.next.lens = *p;
	s.next.shutter.enabled = 0; // (the close lens belonged to the lens that goes)
	return s;
}

inline CameraStep CameraState::set_shutter(const PolarisShutterParams *p) const {
	if (!p || p->struct_size != sizeof(PolarisShutterParams)) return {camera_words("set_shutter: null params or struct_size != %zu", sizeof(PolarisShutterParams)), 0, *this};
	if (p->enabled > 1) return {camera_words("set_shutter: enabled is %u (0 or 1)", p->enabled), 0, *this};
	if (!have_camera) return {"set_shutter: camera not set (the close state belongs to an open one)", 0, *this};
	if (p->enabled && projection_on()) return {"set_shutter: a shutter under a projection other than the perspective one (polaris_hip_set_projection) is not supported", 0, *this};
	if (p->enabled) {
		const float *f = p->eye1; // the 19 camera floats: eye1, frustum1
		for (int i = 0; i < 19; i++)
			if (!std::isfinite(f[i])) return {camera_words("set_shutter: camera float %d is not finite", i), 0, *this};
		if (lens_on()) { // the close lens is a lens that is on, whatever its u1 and v1
			std::string why = check_lens_floats("set_shutter: close lens", &p->focus_distance1, true);
			if (!why.empty()) return {why, 0, *this};
		}
	}
	if (p->enabled ? memcmp(p, &shutter, sizeof shutter) == 0 : !shutter_on()) return {"", 0, *this}; // identical bytes, or off and off: nothing happens
	CameraStep s{"", kCamDropHistory | (p->enabled ? 0u : kCamShutterOff), *this};
	if (p->enabled) s.next.shutter = *p;
	else s.next.shutter.enabled = 0;
	return s;
}

inline CameraStep CameraState::set_projection(const PolarisProjectionParams *p) const {
	if (!p || p->struct_size != sizeof(PolarisProjectionParams))
		return {camera_words("set_projection: null params or struct_size != %zu", sizeof(PolarisProjectionParams)), 0, *this};
	if (p->kind > POLARIS_PROJECTION_EQUIRECTANGULAR) return {camera_words("set_projection: kind is %u (0, 1 or 2)", p->kind), 0, *this};
	if (p->kind == POLARIS_PROJECTION_PERSPECTIVE) { // off: nothing else is looked at, and any two off states are equal
		if (!projection_on()) return {"", 0, *this};
		CameraStep s{"", kCamProjection, *this};
		s.next.projection.kind = POLARIS_PROJECTION_PERSPECTIVE;
		return s;
	}
	if (!have_camera) return {"set_projection: camera not set (the eye is polaris_hip_set_camera's)", 0, *this};
	const float *f = p->axis; // the 13 floats: axis, right, up, half_width, half_height, lon_range, lat_range
	for (int i = 0; i < 13; i++)
		if (!std::isfinite(f[i])) return {camera_words("set_projection: float %d is not finite", i), 0, *this};
	const char *const names[3] = {"axis", "right", "up"};
	for (int k = 0; k < 3; k++) {
		const float *a = f + 3 * k;
		const float a2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
		if (!(a2 >= 0.998f && a2 <= 1.002f)) return {camera_words("set_projection: %s is not a unit vector (squared length %g)", names[k], (double)a2), 0, *this};
	}
	for (int k = 0; k < 3; k++) {
		const float *a = f + 3 * k, *b = f + 3 * ((k + 1) % 3);
		const float ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
		if (!(std::fabs(ab) <= 1e-3f)) return {camera_words("set_projection: %s and %s are not orthogonal (dot %g)", names[k], names[(k + 1) % 3], (double)ab), 0, *this};
	}
	if (p->kind == POLARIS_PROJECTION_ORTHOGRAPHIC) {
		if (!(p->half_width >= 1e-6f && p->half_width <= 1e30f)) return {camera_words("set_projection: half_width %g outside [1e-6, 1e30]", (double)p->half_width), 0, *this};
		if (!(p->half_height >= 1e-6f && p->half_height <= 1e30f)) return {camera_words("set_projection: half_height %g outside [1e-6, 1e30]", (double)p->half_height), 0, *this};
	} else {
		if (!(p->lon_range >= 1e-3f && p->lon_range <= 6.2831855f)) return {camera_words("set_projection: lon_range %g outside [1e-3, 2 pi]", (double)p->lon_range), 0, *this};
		if (!(p->lat_range >= 1e-3f && p->lat_range <= 3.1415927f)) return {camera_words("set_projection: lat_range %g outside [1e-3, pi]", (double)p->lat_range), 0, *this};
	}
	if (lens_on()) return {"set_projection: the lens is on (a lens under a projection other than the perspective one is not supported)", 0, *this};
	if (shutter_on()) return {"set_projection: the shutter is on (a shutter under a projection other than the perspective one is not supported)", 0, *this};
	if (memcmp(p, &projection, sizeof projection) == 0) return {"", 0, *this}; // identical bytes: nothing happens
	CameraStep s{"", kCamProjection, *this};
	s.next.projection = *p;
	return s;
}

} // namespace pol
