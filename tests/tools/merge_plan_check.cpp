// merge_plan_check.cpp -- test tap for merge_plan.h (tests/test_merge_plan_cpu.py): the ring's index rules, the refusals of a block
// request, what an opened peer ring is classified as and the route of a merge, on a CPU.  Everything travels as an int64.
#include "merge_plan.h"

using namespace pol;

extern "C" {

void *ring_new() { return new RingIndex(); }
void ring_delete(void *r) { delete (RingIndex *)r; }
void ring_reset(void *r) { ((RingIndex *)r)->reset(); }
void ring_redepth(void *r, int64_t depth) { ((RingIndex *)r)->redepth((uint32_t)depth); }
void ring_advance(void *r) { ((RingIndex *)r)->advance(); }
int64_t ring_depth(const void *r) { return ((const RingIndex *)r)->depth; }
int64_t ring_pos(const void *r) { return ((const RingIndex *)r)->pos; }
int64_t ring_slot_of(const void *r, int64_t slot) { return ((const RingIndex *)r)->slot_of((int)slot); }
int64_t ring_max_depth() { return POLARIS_IPC_MAX_DEPTH; }

// 0 none, 1 null request, 2 no frame, 3 frame mismatch, 4 rows outside the frame, 5 not full width
int64_t block_refusal(int64_t W, int64_t H, int64_t have_request, int64_t frame_w, int64_t frame_h, int64_t block_x, int64_t block_y, int64_t block_w, int64_t block_h) {
	PolarisBlockRequest r{};
	r.frame_w = (uint32_t)frame_w; r.frame_h = (uint32_t)frame_h;
	r.block_x = (uint32_t)block_x; r.block_y = (uint32_t)block_y; r.block_w = (uint32_t)block_w; r.block_h = (uint32_t)block_h;
	return (int64_t)refuse_block((uint32_t)W, (uint32_t)H, have_request ? &r : nullptr);
}

// out: same_device, local_device, can_access_peer, staged, visible
void peer_class(int64_t have_ids, int64_t same_id, int64_t dst_device, int64_t local_device, int64_t can, int64_t forced, int64_t out[5]) {
	const PeerClass c = classify_peer(have_ids != 0, same_id != 0, (int)dst_device, (int)local_device, (int)can, forced != 0);
	out[0] = c.same_device; out[1] = c.local_device; out[2] = c.can_access_peer; out[3] = c.staged; out[4] = c.visible;
}

// kind: 0 a tracer on dst's GPU, 1 a tracer on another GPU, 2 a mapped peer ring, 3 the caller's device strip.
// out: the POLARIS_MERGE_* branch (-1: no route), how the rows travel (0 in place, 1 peer copy, 2 default copy)
void merge_route(int64_t kind, int64_t same_device, int64_t staged, int64_t can, int64_t enabled, int64_t out[2]) {
	const MergeRoute m = route_merge((MergeKind)kind, (int)same_device, staged != 0, (int)can, enabled != 0);
	out[0] = m.branch; out[1] = (int64_t)m.rows;
}

} // extern "C"
