// trace_plan_projection_check.cpp -- test tap for what TraceScene::projection changes in trace_plan.h (tests/test_trace_plan_projection_cpu.py):
// the plan of one Trace with the lens, the shutter and the projection off and on, from plain numbers, on a CPU.  The fields travel as int64, as in
// trace_plan_check.cpp.
#include "trace_plan.h"

using namespace pol;

extern "C" {

struct ProjectionPlanIn {
	// the options, in the order of TraceOptions
	int64_t samples_per_batch, exact, overlap, packet_shadow, packet_primary, traversal, trace_wgs_per_cu, trace_grid, stage_lds, shade_wave,
	        shade_wgs_per_cu, shade_wave_from, shade_prefilter, shade_sort, hit12, o12;
	// the scene and the device, in the order of TraceScene
	int64_t tiny, resident_closest, resident_any, tables_fit_lds, emit_classes, tri_bits, scene_packet_primary, num_cus, lens, shutter, projection;
	// the request
	int64_t moments, spp, bounces, min_rr, Npad;
};

struct ProjectionPlanOut {
	int64_t K, n_batches, n_pipes, wants_memory_clamp, exact, staged, moments, prefilter, hit12, o12, generate_writes_origins, primary, scene_lens, scene_shutter, scene_projection;
	int64_t isect[POLARIS_MAX_BOUNCES], occl[POLARIS_MAX_BOUNCES], shade[POLARIS_MAX_BOUNCES]; // Traversal / ShadeKernel as numbers
	int64_t grids[3]; // of a full batch: trace_grid(closest), trace_grid(any hit), shade_wave_grid
};

void trace_plan_projection_check(const ProjectionPlanIn *in, ProjectionPlanOut *out) {
	TraceOptions o;
	o.samples_per_batch = in->samples_per_batch; o.exact = (int)in->exact; o.overlap = (int)in->overlap;
	o.packet_shadow = (int)in->packet_shadow; o.packet_primary = (int)in->packet_primary; o.traversal = (int)in->traversal;
	o.trace_wgs_per_cu = (int)in->trace_wgs_per_cu; o.trace_grid = (int)in->trace_grid; o.stage_lds = (int)in->stage_lds;
	o.shade_wave = (int)in->shade_wave; o.shade_wgs_per_cu = (int)in->shade_wgs_per_cu; o.shade_wave_from = (int)in->shade_wave_from;
	o.shade_prefilter = (int)in->shade_prefilter; o.shade_sort = (int)in->shade_sort; o.hit12 = (int)in->hit12; o.o12 = (int)in->o12;
	TraceScene s;
	s.tiny = in->tiny != 0;
	s.resident_per_cu[0] = (int)in->resident_closest; s.resident_per_cu[1] = (int)in->resident_any;
	s.tables_fit_lds = in->tables_fit_lds != 0;
	s.emit_classes = (uint32_t)in->emit_classes; s.tri_bits = (uint32_t)in->tri_bits;
	s.packet_primary = in->scene_packet_primary != 0;
	s.num_cus = (int)in->num_cus;
	s.lens = in->lens != 0;
	s.shutter = in->shutter != 0;
	s.projection = in->projection != 0;
	const TracePlan p = plan_trace(o, s, in->moments != 0, (uint32_t)in->spp, (uint32_t)in->bounces, (uint32_t)in->min_rr, (uint32_t)in->Npad);
	*out = ProjectionPlanOut{};
	out->K = p.K; out->n_batches = p.n_batches; out->n_pipes = p.n_pipes; out->wants_memory_clamp = p.wants_memory_clamp();
	out->exact = p.exact; out->staged = p.staged; out->moments = p.moments; out->prefilter = p.prefilter; out->hit12 = p.hit12; out->o12 = p.o12;
	out->generate_writes_origins = p.generate_writes_origins;
	out->primary = (int64_t)p.primary;
	out->scene_lens = p.scene.lens;
	out->scene_shutter = p.scene.shutter;
	out->scene_projection = p.scene.projection;
	for (int b = 0; b < POLARIS_MAX_BOUNCES; b++) {
		out->isect[b] = b < (int)p.bounces ? (int64_t)p.bounce[b].isect : -1;
		out->occl[b] = b < (int)p.bounces ? (int64_t)p.bounce[b].occl : -1;
		out->shade[b] = b < (int)p.bounces ? (int64_t)p.bounce[b].shade : -1;
	}
	const uint32_t wgs = p.K * (p.Npad / kPlanChunk);
	out->grids[0] = p.trace_grid(false, wgs);
	out->grids[1] = p.trace_grid(true, wgs);
	out->grids[2] = p.shade_wave_grid(wgs);
}

} // extern "C"
