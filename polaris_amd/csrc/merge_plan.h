// merge_plan.h -- the rules behind the accumulators and MergeOutput, as pure host code: where the trace accumulator's ring stands
// (RingIndex), why a block request is refused (refuse_block), what a mapped peer ring is to this process (classify_peer) and how the
// rows of a merge travel and which POLARIS_MERGE_* branch counts them (route_merge).
//
// No HIP here and no device pointer: FrameAccum in polaris_hip.hip owns the buffers, the merge stream and the events, and asks the
// runtime the questions whose answers these functions take; tests/tools/merge_plan_check.cpp asks the same functions on a CPU, where
// every branch can be reached -- on a node whose GPUs all have peer access most of them cannot.  DESIGN.md section 7 describes the paths.
#pragma once

#include <cstdint>

#include "polaris_hip.h"

namespace pol {

// The trace accumulator as a ring of `depth` slots (polaris_hip_ipc_export); `pos` is the slot the last Trace wrote.  Depth 1 is the
// reference's single buffer, which a Trace never leaves.
struct RingIndex {
	uint32_t depth = 1, pos = 0;
	void reset() { depth = 1; pos = 0; }                      // a resize: the ring and its export die with the buffers
	void redepth(uint32_t d) { depth = d; pos %= d; }         // an export of depth d (1..POLARIS_IPC_MAX_DEPTH)
	void advance() { if (depth > 1) pos = (pos + 1) % depth; } // a Trace, behind its last step that can fail for want of memory
	int slot_of(int slot) const { return slot < 0 ? (int)pos : ((uint32_t)slot < depth ? slot : -1); } // slot < 0: the current one; -1: out of range
};

// Why a block request is refused against a W x H frame, in the order the checks are made; every caller words its own message.
enum class BlockRefusal { None, NullRequest, NoFrame, FrameMismatch, RowsOutside, NotFullWidth };
inline BlockRefusal refuse_block(uint32_t W, uint32_t H, const PolarisBlockRequest *r) {
	if (!r) return BlockRefusal::NullRequest;
	if (W == 0 || H == 0) return BlockRefusal::NoFrame;
	if (r->frame_w != W || r->frame_h != H) return BlockRefusal::FrameMismatch;
	if (r->block_h == 0 || (uint64_t)r->block_y + r->block_h > H) return BlockRefusal::RowsOutside;
	if (r->block_x != 0 || (r->block_w != 0 && r->block_w != W)) return BlockRefusal::NotFullWidth; // (BlockW = FrameW, renderer/default.go:110)
	return BlockRefusal::None;
}

// What polaris_hip_ipc_open makes of the exporter's GPU once it has asked the runtime (the first four fields are PolarisPeerInfo's).
struct PeerClass {
	int same_device = -1, local_device = -1, can_access_peer = -1;
	int staged = 0;
	bool visible = true; // false: the ring lives on a GPU this process cannot see -- refused, a peer mapping cannot be verified
};
// have_ids: both sides have a bus id; same_id: and they are equal; dst_device: the opening tracer's; local_device: the exporter's GPU as a
// device index of this process, -1 = none; can: hipDeviceCanAccessPeer(dst_device, local_device), -1 = not asked or the query failed
// (it counts only for another visible GPU); forced: the option "ipc_staged".
// A kernel must never be pointed at memory its device cannot reach (a fault there can take the whole node down), so the ring is read
// where it lies only if it is KNOWN to be reachable: on dst's own GPU, or on one the runtime says it can access.  Anything else -- no
// peer access, a failed query, no bus id -- goes through the staging strip: the runtime moves the rows, the kernel adds a local copy.
inline PeerClass classify_peer(bool have_ids, bool same_id, int dst_device, int local_device, int can, bool forced) {
	PeerClass c;
	if (have_ids) {
		c.same_device = same_id ? 1 : 0;
		c.local_device = same_id ? dst_device : local_device;
		if (!same_id && local_device >= 0 && local_device != dst_device) c.can_access_peer = can;
	}
	c.visible = !(c.same_device == 0 && c.local_device < 0);
	c.staged = (forced || (c.same_device != 1 && c.can_access_peer != 1)) ? 1 : 0;
	return c;
}

// Where the rows of a merge come from, and how they reach the kernel that adds them onto the frame accumulator.
enum class MergeKind { SameDevice, OtherDevice, PeerRing, DeviceStrip }; // a tracer of this process on dst's GPU (dst itself included) | on another GPU | another process's mapped ring | the caller's strip on dst's GPU
enum class RowsTravel { InPlace, PeerCopy, DefaultCopy };                // read where they lie | hipMemcpyPeerAsync into the staging strip | hipMemcpyDefault into it
struct MergeRoute {
	int branch = -1;                       // POLARIS_MERGE_*; -1: no route (OtherDevice whose peer-access query failed: a device error)
	RowsTravel rows = RowsTravel::InPlace;
};
// same_device, staged: the peer's class (PeerRing only).  can, enabled: the answers of hipDeviceCanAccessPeer (1 / 0 / -1 = the query
// failed) and, asked only where can = 1, of hipDeviceEnablePeerAccess -- "already enabled" counts as enabled (OtherDevice only).
inline MergeRoute route_merge(MergeKind kind, int same_device, bool staged, int can, bool enabled) {
	switch (kind) {
	case MergeKind::SameDevice: return {POLARIS_MERGE_LOCAL, RowsTravel::InPlace};
	case MergeKind::OtherDevice:
		if (can < 0) return {};
		if (can == 1 && enabled) return {POLARIS_MERGE_PEER_ACCESS, RowsTravel::InPlace};
		return {POLARIS_MERGE_STAGED, RowsTravel::PeerCopy}; // over xGMI / PCIe, then add
	case MergeKind::PeerRing:
		if (staged || same_device < 0) return {POLARIS_MERGE_IPC_STAGED, RowsTravel::DefaultCopy}; // (an unknown mapping is never read in place: POLARIS_MERGE_IPC_UNKNOWN is no longer counted)
		return {same_device == 1 ? POLARIS_MERGE_IPC_LOCAL : POLARIS_MERGE_IPC_PEER, RowsTravel::InPlace};
	case MergeKind::DeviceStrip: break;
	}
	return {POLARIS_MERGE_DEVICE_STRIP, RowsTravel::InPlace};
}

} // namespace pol
