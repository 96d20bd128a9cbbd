// camera_state_check.cpp -- test tap for camera_state.h (tests/test_camera_state_cpu.py): the three camera setters' transitions, the
// state they leave and the generator it asks for, on a CPU.  The parameter structs travel as the caller's bytes, the state as
// have_camera (a word), the 19 floats of the open camera, PolarisLensParams and PolarisShutterParams, in this order.
#include "camera_state.h"

using namespace pol;

extern "C" {

void *camera_state_new() { return new CameraState(); }
void camera_state_delete(void *s) { delete (CameraState *)s; }

enum Setter { SetCamera, SetLens, SetShutter };

// One setter call as polaris_hip.hip makes it: ask the state, then commit what it returns -- unless it refuses, or commit = 0 (a step
// of the owner's failed).  a, b: SetCamera: eye and frustum; else: the params and nothing.  Returns the CameraTodo bits, -1 for a
// refusal, whose words go to why[cap].
int64_t camera_state_call(void *s, int64_t setter, const void *a, const void *b, int64_t commit, char *why, int64_t cap) {
	CameraState &c = *(CameraState *)s;
	const CameraStep step = setter == SetCamera ? c.set_camera((const float *)a, (const float *)b)
	                        : setter == SetLens ? c.set_lens((const PolarisLensParams *)a) : c.set_shutter((const PolarisShutterParams *)a);
	snprintf(why, (size_t)cap, "%s", step.refusal.c_str());
	if (!step.refusal.empty()) return -1;
	if (commit) c = step.next;
	return step.todo;
}

constexpr int64_t kStateBytes = 4 + 19 * 4 + sizeof(PolarisLensParams) + sizeof(PolarisShutterParams);
int64_t camera_state_bytes(const void *s, uint8_t *out) {
	const CameraState &c = *(const CameraState *)s;
	const uint32_t have = c.have_camera ? 1u : 0u;
	memcpy(out, &have, 4);
	memcpy(out + 4, c.open.eye, 12);
	memcpy(out + 16, c.open.frustum, 64);
	memcpy(out + 80, &c.lens, sizeof c.lens);
	memcpy(out + 80 + sizeof c.lens, &c.shutter, sizeof c.shutter);
	return kStateBytes;
}

// 0 k_generate, 1 k_generate_lens, 2 k_generate_shutter<false>, 3 k_generate_shutter<true>; bit 2: lens_on(), bit 3: shutter_on()
int64_t camera_state_generator(const void *s) {
	const CameraState &c = *(const CameraState *)s;
	return (int64_t)c.generator() | (c.lens_on() ? 4 : 0) | (c.shutter_on() ? 8 : 0);
}

} // extern "C"
