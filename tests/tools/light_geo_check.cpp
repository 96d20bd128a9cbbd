// light_geo_check.cpp -- CPU harness over polaris_amd/csrc/scene_layout.h (test tool, not product).
//
// lg_pack: pack_light_geo over caller arrays, in place over the caller's records.  tests/test_light_geo_cpu.py asserts the records
// equal a numpy float32 restatement, bit for bit.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -Iinclude -Ipolaris_amd/csrc light_geo_check.cpp
#include "scene_layout.h"

extern "C" {

uint32_t lg_record_floats(void) { return pol::kLightGeoFloats; }

// geo: [n][lg_record_floats()], read and written; normals / uvs may be null.
void lg_pack(const PolarisEmissive *ems, uint32_t n, const float *vertices, const float *normals, const float *uvs, float *geo) {
	pol::pack_light_geo(ems, n, vertices, normals, uvs, geo);
}
}
