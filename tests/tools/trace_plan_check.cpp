// trace_plan_check.cpp -- test tap for trace_plan.h (tests/test_trace_plan_cpu.py): the plan of a Trace from plain numbers, on a
// CPU.  Every field travels as an int64 so that the Python side needs one ctypes layout per struct and no padding rules.
#include "trace_plan.h"

using namespace pol;

extern "C" {

struct PlanIn {
	// the options, in the order of TraceOptions
	int64_t samples_per_batch, exact, overlap, packet_shadow, packet_primary, traversal, trace_wgs_per_cu, trace_grid, stage_lds, shade_wave,
	        shade_wgs_per_cu, shade_wave_from, shade_prefilter, shade_sort, hit12, o12;
	// the scene and the device, in the order of TraceScene
	int64_t tiny, resident_closest, resident_any, tables_fit_lds, emit_classes, tri_bits, scene_packet_primary, num_cus;
	// the request
	int64_t moments, spp, bounces, min_rr, Npad;
	// the memory clamp: asked for (as polaris_hip_trace does when the plan wants it and the runtime answers) with `available` = free + held bytes
	int64_t clamp, available;
};

struct PlanOut {
	int64_t K, n_batches, n_pipes, wants_memory_clamp, exact, staged, moments, prefilter, hit12, o12, generate_writes_origins;
	int64_t isect[POLARIS_MAX_BOUNCES], occl[POLARIS_MAX_BOUNCES], shade[POLARIS_MAX_BOUNCES]; // Traversal / ShadeKernel as numbers
};

static TraceOptions options_of(const PlanIn &in) {
	TraceOptions o;
	o.samples_per_batch = in.samples_per_batch; o.exact = (int)in.exact; o.overlap = (int)in.overlap;
	o.packet_shadow = (int)in.packet_shadow; o.packet_primary = (int)in.packet_primary; o.traversal = (int)in.traversal;
	o.trace_wgs_per_cu = (int)in.trace_wgs_per_cu; o.trace_grid = (int)in.trace_grid; o.stage_lds = (int)in.stage_lds;
	o.shade_wave = (int)in.shade_wave; o.shade_wgs_per_cu = (int)in.shade_wgs_per_cu; o.shade_wave_from = (int)in.shade_wave_from;
	o.shade_prefilter = (int)in.shade_prefilter; o.shade_sort = (int)in.shade_sort; o.hit12 = (int)in.hit12; o.o12 = (int)in.o12;
	return o;
}

static TraceScene scene_of(const PlanIn &in) {
	TraceScene s;
	s.tiny = in.tiny != 0;
	s.resident_per_cu[0] = (int)in.resident_closest; s.resident_per_cu[1] = (int)in.resident_any;
	s.tables_fit_lds = in.tables_fit_lds != 0;
	s.emit_classes = (uint32_t)in.emit_classes; s.tri_bits = (uint32_t)in.tri_bits;
	s.packet_primary = in.scene_packet_primary != 0;
	s.num_cus = (int)in.num_cus;
	return s;
}

static TracePlan plan_of(const PlanIn &in) {
	TracePlan p = plan_trace(options_of(in), scene_of(in), in.moments != 0, (uint32_t)in.spp, (uint32_t)in.bounces, (uint32_t)in.min_rr, (uint32_t)in.Npad);
	if (in.clamp && p.wants_memory_clamp()) p.clamp_to_memory((size_t)in.available);
	return p;
}

static void report(const TracePlan &p, PlanOut *out) {
	*out = PlanOut{};
	out->K = p.K; out->n_batches = p.n_batches; out->n_pipes = p.n_pipes; out->wants_memory_clamp = p.wants_memory_clamp();
	out->exact = p.exact; out->staged = p.staged; out->moments = p.moments; out->prefilter = p.prefilter; out->hit12 = p.hit12; out->o12 = p.o12;
	out->generate_writes_origins = p.generate_writes_origins;
	for (int b = 0; b < POLARIS_MAX_BOUNCES; b++) {
		out->isect[b] = b < (int)p.bounces ? (int64_t)p.bounce[b].isect : -1;
		out->occl[b] = b < (int)p.bounces ? (int64_t)p.bounce[b].occl : -1;
		out->shade[b] = b < (int)p.bounces ? (int64_t)p.bounce[b].shade : -1;
	}
}

void trace_plan_check(const PlanIn *in, PlanOut *out) { report(plan_of(*in), out); }

// The plan after `shrinks` failed allocations; returns how many of them the plan answered with a smaller K (fewer: the failure was final).
int64_t trace_plan_shrunk(const PlanIn *in, int64_t shrinks, PlanOut *out) {
	TracePlan p = plan_of(*in);
	int64_t taken = 0;
	while (taken < shrinks && p.shrink()) taken++;
	report(p, out);
	return taken;
}

int64_t trace_plan_bytes_needed(const PlanIn *in, int64_t k) { return (int64_t)plan_of(*in).bytes_needed((uint32_t)k); }
int64_t trace_plan_slot_bytes(int64_t nee_bounces) { return (int64_t)slot_bytes((uint32_t)nee_bounces); }

// grids[0 .. 2]: the persistent traversal grids (closest hit, any hit) and the k_shade_wave grid of a launch of `wgs` chunks
void trace_plan_grids(const PlanIn *in, int64_t wgs, int64_t grids[3]) {
	const TracePlan p = plan_of(*in);
	grids[0] = p.trace_grid(false, (uint32_t)wgs);
	grids[1] = p.trace_grid(true, (uint32_t)wgs);
	grids[2] = p.shade_wave_grid((uint32_t)wgs);
}

// The traversal choice outside a batch: kind = RayKind as a number.
int64_t trace_plan_batch_traversal(const PlanIn *in, int64_t kind, int64_t bounce) { return (int64_t)batch_traversal(options_of(*in), scene_of(*in), (RayKind)kind, (uint32_t)bounce); }
int64_t trace_plan_probe_traversal(const PlanIn *in, int64_t kind) { return (int64_t)probe_traversal(options_of(*in), (RayKind)kind); }
int64_t trace_plan_tap_traversal(const PlanIn *in) { return (int64_t)tap_traversal(scene_of(*in)); }
int64_t trace_plan_probe_grid(const PlanIn *in, int64_t any_hit, int64_t wgs) { return probe_grid(scene_of(*in), any_hit != 0, (uint32_t)wgs); }
const char *trace_plan_timer(int64_t how, int64_t kind) { return traversal_timer((Traversal)how, (RayKind)kind); }
int64_t trace_plan_tables_staged(const PlanIn *in) { return tables_staged(options_of(*in), scene_of(*in)); }

} // extern "C"
