// projection_state_check.cpp -- a stand-alone program that drives CameraState (polaris_amd/csrc/camera_state.h) through a script of
// setter calls, for tests/test_projection_state_cpu.py, which compares every answer with a model.  Built as a plain host program with
// -fsanitize=address,undefined.  With -DPOLARIS_NO_PROJECTION it compiles against a camera_state.h that knows no projection (the test
// builds it against the header of the commit before polaris_hip_set_projection) and prints the same lines without the projection's fields.
//
// stdin, one call per line: a letter and the caller's bytes in hex --
//   C <eye 12 bytes><frustum 64 bytes>   set_camera        L <PolarisLensParams>   set_lens      S <PolarisShutterParams>   set_shutter
//   P <PolarisProjectionParams>          set_projection    a letter followed by "null": the call with null params
//   a letter in lower case: the same call, not committed (a step of the owner's failed)
// stdout, one line per call: todo (-1: refused) | generator | lens_on shutter_on [projection_on] | the state's bytes in hex | the refusal's words
#include <iostream>
#include <sstream>
#include <vector>

#include "camera_state.h"

using namespace pol;

static std::vector<uint8_t> unhex(const std::string &s) {
	std::vector<uint8_t> out;
	for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
	return out;
}
static void hex(const void *p, size_t n) {
	static const char digits[] = "0123456789abcdef";
	const uint8_t *b = (const uint8_t *)p;
	for (size_t i = 0; i < n; i++) std::cout << digits[b[i] >> 4] << digits[b[i] & 15];
}

int main() {
	CameraState c;
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty()) continue;
		std::istringstream in(line);
		std::string op, arg;
		in >> op >> arg;
		const char what = (char)std::toupper((unsigned char)op[0]);
		const bool commit = what == op[0], null = arg == "null";
		// the caller's bytes in a heap block of exactly their size: a read past the struct is the sanitizer's to report
		const std::vector<uint8_t> bytes = null ? std::vector<uint8_t>() : unhex(arg);
		std::vector<uint8_t> *heap = null ? nullptr : new std::vector<uint8_t>(bytes);
		const void *p = heap ? heap->data() : nullptr;
		CameraStep step;
		if (what == 'C') step = null ? c.set_camera(nullptr, nullptr) : c.set_camera((const float *)p, (const float *)p + 3);
		else if (what == 'L') step = c.set_lens((const PolarisLensParams *)p);
		else if (what == 'S') step = c.set_shutter((const PolarisShutterParams *)p);
#ifndef POLARIS_NO_PROJECTION
		else if (what == 'P') step = c.set_projection((const PolarisProjectionParams *)p);
#endif
		else { std::cerr << "unknown call " << op << "\n"; return 2; }
		delete heap;
		const bool refused = !step.refusal.empty();
		if (!refused && commit) c = step.next;
		std::cout << (refused ? -1 : (int)step.todo) << "|" << (int)c.generator() << "|" << c.lens_on() << " " << c.shutter_on();
#ifndef POLARIS_NO_PROJECTION
		std::cout << " " << c.projection_on();
#endif
		std::cout << "|";
		const uint32_t have = c.have_camera ? 1u : 0u;
		hex(&have, 4); hex(c.open.eye, 12); hex(c.open.frustum, 64); hex(&c.lens, sizeof c.lens); hex(&c.shutter, sizeof c.shutter);
#ifndef POLARIS_NO_PROJECTION
		hex(&c.projection, sizeof c.projection);
#endif
		std::cout << "|" << step.refusal << "\n";
	}
	return 0;
}
