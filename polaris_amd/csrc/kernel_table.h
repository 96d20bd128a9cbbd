// kernel_table.h -- every kernel the host launches under a timer, named ONCE (host code only).
//
// A Variant is a kernel's function pointer, typed with the kernel family's own signature, next to the symbol the profiler prints
// for it.  Both come from one spelling of the template-id (POLARIS_VARIANT): the string polaris_hip_kernel_symbol reports, by which
// bench.py names its roofline objects, cannot disagree with the kernel that ran, and the compiler checks a launch through the
// pointer against the kernel's parameter list.  The tables list exactly the instantiations the library holds.
#pragma once

#include <utility>

#include "kernels.h"
#include "instance_update.h"
#include "vertex_update.h"
#include "material_update.h"

namespace pol {

template <class... P>
struct Variant {
	void (*fn)(P...);
	const char *symbol;
	constexpr Variant(void (*f)(P...), const char *s) : fn(f), symbol(s) {}
	const void *address() const { return reinterpret_cast<const void *>(fn); } // what the occupancy and attribute calls take
	template <class... A> // (a launch's error is left for hipGetLastError / hipPeekAtLastError)
	void enqueue(dim3 grid, uint32_t block, uint32_t lds_bytes, hipStream_t q, A &&...a) const { // (grid: a count, or a dim3)
		fn<<<grid, dim3(block), lds_bytes, q>>>(std::forward<A>(a)...);
	}
};
// Spell EVERY template argument, defaults included, NODES as its number: that is how the profiler prints the symbol.
#define POLARIS_VARIANT(...) Variant(&pol::__VA_ARGS__, "pol::" #__VA_ARGS__)
static_assert(kNodesGlobal == 0 && kNodesLdsTop == 1 && kNodesLdsAll == 2, "the k_trace entries below spell NODES as a number");

// k_trace<ANY_HIT, STACK, NODES, ONE>: [any hit][stack 16 / 24 / 32][node records global / LDS top]; tiny-scene mode: [any hit][general / ONE]
using TraceVariant = decltype(POLARIS_VARIANT(k_trace<false, 16, 0, false>));
const TraceVariant kTrace[2][3][2] = {
	{{POLARIS_VARIANT(k_trace<false, 16, 0, false>), POLARIS_VARIANT(k_trace<false, 16, 1, false>)},
	 {POLARIS_VARIANT(k_trace<false, 24, 0, false>), POLARIS_VARIANT(k_trace<false, 24, 1, false>)},
	 {POLARIS_VARIANT(k_trace<false, 32, 0, false>), POLARIS_VARIANT(k_trace<false, 32, 1, false>)}},
	{{POLARIS_VARIANT(k_trace<true, 16, 0, false>), POLARIS_VARIANT(k_trace<true, 16, 1, false>)},
	 {POLARIS_VARIANT(k_trace<true, 24, 0, false>), POLARIS_VARIANT(k_trace<true, 24, 1, false>)},
	 {POLARIS_VARIANT(k_trace<true, 32, 0, false>), POLARIS_VARIANT(k_trace<true, 32, 1, false>)}}};
const TraceVariant kTraceTiny[2][2] = {{POLARIS_VARIANT(k_trace<false, 16, 2, false>), POLARIS_VARIANT(k_trace<false, 16, 2, true>)},
                                       {POLARIS_VARIANT(k_trace<true, 16, 2, false>), POLARIS_VARIANT(k_trace<true, 16, 2, true>)}};
// The k_trace variant of the uploaded scene with what its launch needs, resolved once per upload (polaris_hip.hip, select_trace).
struct TraceLaunch {
	const TraceVariant *v = nullptr;
	int block = WG;          // workgroup size (kTinyBlock in the tiny-scene mode)
	uint32_t lds_bytes = 0;  // dynamic LDS block of a workgroup (tiny-scene mode: stack rows + tree + triangle records, plan_tiny_lds)
	int resident_per_cu = 6; // workgroups of it a CU holds at once (occupancy API)
};

// k_shade<LDS, SORT, FIRST>: [LDS tables][first / sort / plain], the order of the shade timers; k_shade_wave<LDS>: [LDS tables]
using ShadeVariant = decltype(POLARIS_VARIANT(k_shade<false, false, true>));
const ShadeVariant kShade[2][3] = {
	{POLARIS_VARIANT(k_shade<false, false, true>), POLARIS_VARIANT(k_shade<false, true, false>), POLARIS_VARIANT(k_shade<false, false, false>)},
	{POLARIS_VARIANT(k_shade<true, false, true>), POLARIS_VARIANT(k_shade<true, true, false>), POLARIS_VARIANT(k_shade<true, false, false>)}};
using ShadeWaveVariant = decltype(POLARIS_VARIANT(k_shade_wave<false>));
const ShadeWaveVariant kShadeWave[2] = {POLARIS_VARIANT(k_shade_wave<false>), POLARIS_VARIANT(k_shade_wave<true>)};

// k_trace_packet<ANY_HIT, CAMERA>
using PacketVariant = decltype(POLARIS_VARIANT(k_trace_packet<false, true>));
enum { kPacketCamera, kPacketClosest, kPacketAnyHit };
const PacketVariant kPacket[3] = {POLARIS_VARIANT(k_trace_packet<false, true>), POLARIS_VARIANT(k_trace_packet<false, false>),
                                  POLARIS_VARIANT(k_trace_packet<true, false>)};

// the kernels of two variants: [MOMENTS]; k_reproject<M2, MOTION>: [M2][MOTION]
const decltype(POLARIS_VARIANT(k_resolve<false>)) kResolve[2] = {POLARIS_VARIANT(k_resolve<false>), POLARIS_VARIANT(k_resolve<true>)};
const decltype(POLARIS_VARIANT(k_aggregate<false>)) kAggregate[2] = {POLARIS_VARIANT(k_aggregate<false>), POLARIS_VARIANT(k_aggregate<true>)};
const decltype(POLARIS_VARIANT(k_reproject<false, false>)) kReproject[2][2] = {
	{POLARIS_VARIANT(k_reproject<false, false>), POLARIS_VARIANT(k_reproject<false, true>)},
	{POLARIS_VARIANT(k_reproject<true, false>), POLARIS_VARIANT(k_reproject<true, true>)}};
// k_reproject_deform<M2>: [M2].  Option "vertex_motion": in k_reproject<M2, true>'s place while the history has a snapshot of the vertices
const decltype(POLARIS_VARIANT(k_reproject_deform<false>)) kReprojectDeform[2] = {POLARIS_VARIANT(k_reproject_deform<false>), POLARIS_VARIANT(k_reproject_deform<true>)};
// k_generate_shutter<LENS>: [LENS].  polaris_hip_set_shutter: in k_generate's (k_generate_lens') place while the shutter is on
const decltype(POLARIS_VARIANT(k_generate_shutter<false>)) kGenerateShutter[2] = {POLARIS_VARIANT(k_generate_shutter<false>), POLARIS_VARIANT(k_generate_shutter<true>)};
// polaris_hip_set_projection, while the projection is on: k_generate_proj<PROJ>: [kind - 1] in k_generate's place,
// k_gbuffer_proj / k_gbuffer_chain_proj in the G-buffer kernels', k_reproject_proj<M2, MOTION> and k_reproject_deform_proj<M2> in the reprojection's
const decltype(POLARIS_VARIANT(k_generate_proj<1>)) kGenerateProj[2] = {POLARIS_VARIANT(k_generate_proj<1>), POLARIS_VARIANT(k_generate_proj<2>)};
static_assert(POLARIS_PROJECTION_ORTHOGRAPHIC == 1 && POLARIS_PROJECTION_EQUIRECTANGULAR == 2 && kTpOrthographic == 1 && kTpEquirectangular == 2,
              "kGenerateProj spells PROJ as a number");
const auto kGbufferProj = POLARIS_VARIANT(k_gbuffer_proj);
const auto kGbufferChainProj = POLARIS_VARIANT(k_gbuffer_chain_proj);
const decltype(POLARIS_VARIANT(k_reproject_proj<false, false>)) kReprojectProj[2][2] = {
	{POLARIS_VARIANT(k_reproject_proj<false, false>), POLARIS_VARIANT(k_reproject_proj<false, true>)},
	{POLARIS_VARIANT(k_reproject_proj<true, false>), POLARIS_VARIANT(k_reproject_proj<true, true>)}};
const decltype(POLARIS_VARIANT(k_reproject_deform_proj<false>)) kReprojectDeformProj[2] = {POLARIS_VARIANT(k_reproject_deform_proj<false>),
                                                                                         POLARIS_VARIANT(k_reproject_deform_proj<true>)};

// the kernels of one variant (k_intersect / k_occlusion: the plain traversal, option traversal = 0)
const auto kIntersect = POLARIS_VARIANT(k_intersect);
const auto kOcclusion = POLARIS_VARIANT(k_occlusion);
const auto kGenerate = POLARIS_VARIANT(k_generate);
const auto kGenerateLens = POLARIS_VARIANT(k_generate_lens); // polaris_hip_set_lens: in k_generate's place while the lens is on
const auto kScan = POLARIS_VARIANT(k_scan);
const auto kFoldNee = POLARIS_VARIANT(k_fold_nee);
const auto kTonemap = POLARIS_VARIANT(k_tonemap);
const auto kGbuffer = POLARIS_VARIANT(k_gbuffer);
const auto kGbufferChain = POLARIS_VARIANT(k_gbuffer_chain); // option "guide_specular" > 0: in k_gbuffer's place
const auto kDenoise = POLARIS_VARIANT(k_denoise);
const auto kTemporal = POLARIS_VARIANT(k_temporal);
const auto kVariance = POLARIS_VARIANT(k_variance);
const auto kDenoiseVariance = POLARIS_VARIANT(k_denoise_variance);
// polaris_hip_set_display (display.h): k_display<OP, SRGB>: [tone operator][srgb]
const auto kMeter = POLARIS_VARIANT(k_meter);
const auto kExpose = POLARIS_VARIANT(k_expose);
const decltype(POLARIS_VARIANT(k_display<0, false>)) kDisplay[4][2] = {
	{POLARIS_VARIANT(k_display<0, false>), POLARIS_VARIANT(k_display<0, true>)}, {POLARIS_VARIANT(k_display<1, false>), POLARIS_VARIANT(k_display<1, true>)},
	{POLARIS_VARIANT(k_display<2, false>), POLARIS_VARIANT(k_display<2, true>)}, {POLARIS_VARIANT(k_display<3, false>), POLARIS_VARIANT(k_display<3, true>)}};
static_assert(POLARIS_TONE_REINHARD == 0 && POLARIS_TONE_REINHARD_WHITE == 1 && POLARIS_TONE_ACES == 2 && POLARIS_TONE_HABLE == 3, "kDisplay spells OP as a number");
// polaris_hip_set_bloom (bloom.h): k_bloom_down<FIRST, KARIS> and k_bloom_tail<FIRST, KARIS>: [0 a coarser level, 1 level 1, 2 level 1 with karis];
// k_display_bloom<OP, SRGB> as kDisplay
const decltype(POLARIS_VARIANT(k_bloom_down<false, false>)) kBloomDown[3] = {POLARIS_VARIANT(k_bloom_down<false, false>), POLARIS_VARIANT(k_bloom_down<true, false>),
                                                                             POLARIS_VARIANT(k_bloom_down<true, true>)};
const decltype(POLARIS_VARIANT(k_bloom_tail<false, false>)) kBloomTail[3] = {POLARIS_VARIANT(k_bloom_tail<false, false>), POLARIS_VARIANT(k_bloom_tail<true, false>),
                                                                             POLARIS_VARIANT(k_bloom_tail<true, true>)};
const auto kBloomUp = POLARIS_VARIANT(k_bloom_up);
const decltype(POLARIS_VARIANT(k_display_bloom<0, false>)) kDisplayBloom[4][2] = {
	{POLARIS_VARIANT(k_display_bloom<0, false>), POLARIS_VARIANT(k_display_bloom<0, true>)}, {POLARIS_VARIANT(k_display_bloom<1, false>), POLARIS_VARIANT(k_display_bloom<1, true>)},
	{POLARIS_VARIANT(k_display_bloom<2, false>), POLARIS_VARIANT(k_display_bloom<2, true>)}, {POLARIS_VARIANT(k_display_bloom<3, false>), POLARIS_VARIANT(k_display_bloom<3, true>)}};
// polaris_hip_update_instances (instance_update.h)
const auto kInstanceExtent = POLARIS_VARIANT(k_instance_extent);
const auto kRepad = POLARIS_VARIANT(k_repad);
const auto kRefitTop = POLARIS_VARIANT(k_refit_top);
// polaris_hip_update_vertices (vertex_update.h)
const auto kTriRecords = POLARIS_VARIANT(k_tri_records);
const auto kRefitMesh = POLARIS_VARIANT(k_refit_mesh);
// polaris_hip_update_materials (material_update.h)
const auto kRetag = POLARIS_VARIANT(k_retag);
const auto kEmissiveNodes = POLARIS_VARIANT(k_emissive_nodes);

} // namespace pol
