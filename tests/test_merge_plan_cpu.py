"""CPU test of the rules behind the accumulators and MergeOutput (polaris_amd/csrc/merge_plan.h): where the trace accumulator's ring
stands after every event, why a block request is refused, what polaris_hip_ipc_open makes of the runtime's answers about a peer's
GPU, and how the rows of a merge travel and which POLARIS_MERGE_* branch counts them.

tests/tools/merge_plan_check.cpp hands plain numbers to the header.  Every expectation below is written out by hand from DESIGN.md
section 7 and the host code before the header existed; none is read back from the library.  Most of these branches cannot be reached
on a node whose GPUs all have peer access and bus ids -- and they are the ones where a mistake points a kernel at memory its device
cannot reach -- which is why they are tested here and not on a GPU.
"""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "merge_plan_check.cpp")
LIB = os.path.join(BUILD, "libmerge_plan_check.so")

MAX_DEPTH = 4                                                                          # POLARIS_IPC_MAX_DEPTH
NONE, NULL_REQUEST, NO_FRAME, FRAME_MISMATCH, ROWS_OUTSIDE, NOT_FULL_WIDTH = range(6)  # BlockRefusal, in the order of the checks
LOCAL, PEER_ACCESS, STAGED, IPC_LOCAL, IPC_PEER, IPC_UNKNOWN, DEVICE_STRIP, IPC_STAGED = range(8)   # POLARIS_MERGE_*
SAME_DEVICE, OTHER_DEVICE, PEER_RING, DEVICE_STRIP_KIND = range(4)                     # MergeKind
IN_PLACE, PEER_COPY, DEFAULT_COPY = range(3)                                           # RowsTravel
NO_ROUTE = -1


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "merge_plan.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    so = C.CDLL(LIB)
    so.ring_new.restype = C.c_void_p
    for name in ("ring_delete", "ring_reset", "ring_redepth", "ring_advance", "peer_class", "merge_route"):
        getattr(so, name).restype = None
    for name in ("ring_depth", "ring_pos", "ring_slot_of", "ring_max_depth", "block_refusal"):
        getattr(so, name).restype = C.c_int64
    return so


# ---- the ring

class Ring:
    def __init__(self, lib):
        self.lib, self.r = lib, C.c_void_p(lib.ring_new())

    def close(self):
        self.lib.ring_delete(self.r)

    def reset(self):
        self.lib.ring_reset(self.r)

    def redepth(self, d):
        self.lib.ring_redepth(self.r, C.c_int64(d))

    def advance(self):
        self.lib.ring_advance(self.r)
        return self.state()[1]

    def state(self):
        return (self.lib.ring_depth(self.r), self.lib.ring_pos(self.r))

    def slot_of(self, slot):
        return self.lib.ring_slot_of(self.r, C.c_int64(slot))


@pytest.fixture
def ring(lib):
    r = Ring(lib)
    yield r
    r.close()


def test_ring_index_rules(lib, ring):
    assert lib.ring_max_depth() == MAX_DEPTH
    assert ring.state() == (1, 0)                                    # a fresh ring: the reference's single buffer
    assert [ring.advance() for _ in range(3)] == [0, 0, 0]           # which a Trace never leaves
    assert ring.slot_of(-1) == 0 and ring.slot_of(0) == 0 and ring.slot_of(1) == -1
    ring.redepth(3)
    assert ring.state() == (3, 0)
    assert [ring.advance() for _ in range(4)] == [1, 2, 0, 1]
    ring.advance()
    assert ring.state() == (3, 2) and ring.slot_of(-1) == 2          # slot < 0: the current one
    assert [ring.slot_of(s) for s in (0, 1, 2)] == [0, 1, 2]         # (depth - 1 is accepted)
    assert ring.slot_of(3) == -1 and ring.slot_of(MAX_DEPTH) == -1   # depth and POLARIS_IPC_MAX_DEPTH are refused
    ring.redepth(2)                                                  # 3 -> 2 from pos 2: pos %= depth
    assert ring.state() == (2, 0) and ring.slot_of(2) == -1
    ring.reset()
    assert ring.state() == (1, 0)
    ring.redepth(4)                                                  # 1 -> 4 keeps pos 0
    assert ring.state() == (4, 0) and ring.slot_of(3) == 3 and ring.slot_of(MAX_DEPTH) == -1
    assert [ring.advance() for _ in range(5)] == [1, 2, 3, 0, 1]
    ring.redepth(1)
    assert ring.state() == (1, 0) and ring.advance() == 0
    ring.redepth(3)
    ring.advance()
    ring.reset()
    assert ring.state() == (1, 0) and ring.slot_of(-1) == 0 and ring.slot_of(1) == -1


class RingModel:
    """The ring of tests/test_gpu_api_sequences.py's Model, restated: resize, export and the advance of do_trace."""

    def __init__(self):
        self.resize()

    def resize(self):
        self.depth, self.pos = 1, 0

    def export(self, depth):
        self.depth = depth
        self.pos %= depth

    def trace(self):
        if self.depth > 1:
            self.pos = (self.pos + 1) % self.depth


@pytest.mark.parametrize("seed", range(4))
def test_ring_random_walk_against_the_model(ring, seed):
    rng = random.Random(0xA11CE + seed)
    m = RingModel()
    for step in range(400):
        op = rng.choice(["trace", "trace", "trace", "export", "resize"])
        if op == "trace":
            ring.advance()
            m.trace()
        elif op == "export":
            d = rng.randint(1, MAX_DEPTH)
            ring.redepth(d)
            m.export(d)
        else:
            ring.reset()
            m.resize()
        assert ring.state() == (m.depth, m.pos), (seed, step, op)
        for s in range(-2, MAX_DEPTH + 2):
            assert ring.slot_of(s) == (m.pos if s < 0 else (s if s < m.depth else -1)), (seed, step, s)


# ---- the refusals of a block request

W, H = 33, 17


def refusal(lib, W=W, H=H, have_request=1, frame_w=W, frame_h=H, block_x=0, block_y=0, block_w=W, block_h=H):
    return lib.block_refusal(*(C.c_int64(v) for v in (W, H, have_request, frame_w, frame_h, block_x, block_y, block_w, block_h)))


def test_block_refusals_one_per_reason(lib):
    assert refusal(lib) == NONE
    assert refusal(lib, have_request=0) == NULL_REQUEST
    assert refusal(lib, W=0, H=0, frame_w=0, frame_h=0) == NO_FRAME
    assert refusal(lib, W=0) == NO_FRAME and refusal(lib, H=0) == NO_FRAME
    assert refusal(lib, frame_w=W + 1) == FRAME_MISMATCH and refusal(lib, frame_h=H - 1) == FRAME_MISMATCH
    assert refusal(lib, block_h=0) == ROWS_OUTSIDE                              # an empty block
    assert refusal(lib, block_y=1) == ROWS_OUTSIDE                              # rows [1, H + 1)
    assert refusal(lib, block_y=H, block_h=1) == ROWS_OUTSIDE
    assert refusal(lib, block_y=H - 1, block_h=1) == NONE                       # the last row alone
    assert refusal(lib, block_x=1) == NOT_FULL_WIDTH


def test_block_refusals_in_order_of_precedence(lib):
    """A request wrong in two ways reports the earlier check."""
    assert refusal(lib, have_request=0, W=0, H=0) == NULL_REQUEST
    assert refusal(lib, W=0, H=0, block_h=0) == NO_FRAME                        # (its frame does not match either)
    assert refusal(lib, frame_w=W + 1, block_y=H) == FRAME_MISMATCH
    assert refusal(lib, frame_h=H + 1, block_x=3) == FRAME_MISMATCH
    assert refusal(lib, block_h=0, block_x=1) == ROWS_OUTSIDE
    assert refusal(lib, block_y=H, block_w=W - 1) == ROWS_OUTSIDE


def test_block_rows_are_summed_in_64_bits(lib):
    assert refusal(lib, block_y=0xFFFFFFF0, block_h=0x20) == ROWS_OUTSIDE        # (the 32-bit sum is 0x10: inside a frame of 17 rows)
    assert refusal(lib, W=8, H=0xFFFFFFFF, frame_w=8, frame_h=0xFFFFFFFF, block_w=8, block_y=0xFFFFFFF0, block_h=0xF) == NONE
    assert refusal(lib, W=8, H=0xFFFFFFFF, frame_w=8, frame_h=0xFFFFFFFF, block_w=8, block_y=0xFFFFFFF0, block_h=0x10) == ROWS_OUTSIDE


def test_block_width_is_the_frame_or_zero(lib):
    assert refusal(lib, block_w=0) == NONE and refusal(lib, block_w=W) == NONE
    assert refusal(lib, block_w=W - 1) == NOT_FULL_WIDTH and refusal(lib, block_w=W + 1) == NOT_FULL_WIDTH and refusal(lib, block_w=1) == NOT_FULL_WIDTH


# ---- what an opened peer ring is

DST, OTHER = 2, 5          # the opening tracer's device index; the exporter's GPU as another device index of this process


def classify(lib, have_ids, same_id, local, can, forced):
    out = (C.c_int64 * 5)()
    lib.peer_class(*(C.c_int64(v) for v in (have_ids, same_id, DST, local, can, forced)), out)
    return dict(same=out[0], local=out[1], can=out[2], staged=out[3], visible=bool(out[4]))


def peer_rule(have_ids, same_id, local, can, forced, parent=False):
    """polaris_hip_ipc_open, restated.  parent: `staged` as it was decided before an unknown mapping went through the strip."""
    if not have_ids:                       # no bus id on either side: nothing is known, nothing was asked
        same, loc, c = -1, -1, -1
    elif same_id:                          # dst's own GPU: peer access is not asked
        same, loc, c = 1, DST, -1
    else:                                  # another GPU: can-access counts where it is visible
        same, loc, c = 0, local, (can if local >= 0 and local != DST else -1)
    visible = not (same == 0 and loc < 0)
    if parent:
        staged = bool(forced) or (same == 0 and c == 0)
    else:                                  # read in place only what is KNOWN to be reachable
        staged = bool(forced) or (same != 1 and c != 1)
    return dict(same=same, local=loc, can=c, staged=int(staged), visible=visible)


PEER_PRODUCT = list(itertools.product((0, 1), (0, 1), (-1, OTHER), (1, 0, -1), (0, 1)))   # bus ids present, equal, local device found, can-access, forced


@pytest.mark.parametrize("have_ids, same_id, local, can, forced", PEER_PRODUCT)
def test_peer_classification(lib, have_ids, same_id, local, can, forced):
    got = classify(lib, have_ids, same_id, local, can, forced)
    assert got == peer_rule(have_ids, same_id, local, can, forced), (have_ids, same_id, local, can, forced)
    if got["staged"] == 0:                 # read where it lies: only dst's own GPU, or a visible one the runtime says it can access
        assert got["same"] == 1 or (got["same"] == 0 and got["local"] == OTHER and got["can"] == 1)


def test_peer_classification_named_rows(lib):
    assert classify(lib, 1, 1, OTHER, 0, 0) == dict(same=1, local=DST, can=-1, staged=0, visible=True)       # dst's own GPU: never asked, never staged ...
    assert classify(lib, 1, 1, OTHER, 0, 1)["staged"] == 1                                                  # ... unless forced
    assert classify(lib, 1, 0, -1, -1, 0)["visible"] is False and classify(lib, 1, 0, -1, 1, 1)["visible"] is False   # not visible: refused, forced or not
    assert classify(lib, 1, 0, OTHER, 1, 0) == dict(same=0, local=OTHER, can=1, staged=0, visible=True)      # peer access: read in place
    assert classify(lib, 1, 0, OTHER, 0, 0) == dict(same=0, local=OTHER, can=0, staged=1, visible=True)      # none: the strip
    # the two rows that an unknown mapping flips, by name
    no_bus_id = classify(lib, 0, 0, -1, -1, 0)
    assert no_bus_id == dict(same=-1, local=-1, can=-1, staged=1, visible=True) and peer_rule(0, 0, -1, -1, 0, parent=True)["staged"] == 0
    query_failed = classify(lib, 1, 0, OTHER, -1, 0)
    assert query_failed == dict(same=0, local=OTHER, can=-1, staged=1, visible=True) and peer_rule(1, 0, OTHER, -1, 0, parent=True)["staged"] == 0


def test_only_the_unknown_mappings_flip(lib):
    """Against the rule as it was: `staged` differs for exactly the mappings that are opened (visible, not forced) with nothing known
    of their reachability -- no bus id, or a visible GPU whose can-access query failed -- and nothing else differs anywhere."""
    flipped = set()
    for row in PEER_PRODUCT:
        new, old = peer_rule(*row), peer_rule(*row, parent=True)
        assert {k: v for k, v in new.items() if k != "staged"} == {k: v for k, v in old.items() if k != "staged"}
        if not new["visible"]:             # refused: no peer comes of it, `staged` says nothing
            continue
        if new["staged"] != old["staged"]:
            assert (old["staged"], new["staged"]) == (0, 1) and not row[4]
            flipped.add((new["same"], new["local"], new["can"]))
    assert flipped == {(-1, -1, -1), (0, OTHER, -1)}


# ---- the route of a merge

def route(lib, kind, same_device=-1, staged=0, can=-1, enabled=0):
    out = (C.c_int64 * 2)()
    lib.merge_route(*(C.c_int64(v) for v in (kind, same_device, staged, can, enabled)), out)
    return (out[0], out[1])


def test_route_of_a_tracer_of_this_process(lib):
    for can, enabled in itertools.product((1, 0, -1), (0, 1)):               # the same GPU: whatever the runtime would say
        assert route(lib, SAME_DEVICE, can=can, enabled=enabled) == (LOCAL, IN_PLACE)
    assert route(lib, OTHER_DEVICE, can=1, enabled=1) == (PEER_ACCESS, IN_PLACE)   # (hipErrorPeerAccessAlreadyEnabled counts as enabled)
    assert route(lib, OTHER_DEVICE, can=1, enabled=0) == (STAGED, PEER_COPY)       # enabling failed
    assert route(lib, OTHER_DEVICE, can=0, enabled=0) == (STAGED, PEER_COPY)
    assert route(lib, OTHER_DEVICE, can=0, enabled=1) == (STAGED, PEER_COPY)       # (not asked where can = 0: ignored)
    for enabled in (0, 1):                                                         # a failed query is an error, not a route
        assert route(lib, OTHER_DEVICE, can=-1, enabled=enabled)[0] == NO_ROUTE
    for same, staged in itertools.product((1, 0, -1), (0, 1)):                     # (a peer's class says nothing about a tracer)
        assert route(lib, OTHER_DEVICE, same, staged, can=1, enabled=1) == (PEER_ACCESS, IN_PLACE)
        assert route(lib, SAME_DEVICE, same, staged) == (LOCAL, IN_PLACE)


def test_route_of_a_peer_ring_and_of_a_device_strip(lib):
    for can, enabled in itertools.product((1, 0, -1), (0, 1)):                     # (asked at ipc_open, not at the merge)
        assert route(lib, PEER_RING, 1, 0, can, enabled) == (IPC_LOCAL, IN_PLACE)
        assert route(lib, PEER_RING, 0, 0, can, enabled) == (IPC_PEER, IN_PLACE)
        for same in (1, 0, -1):
            assert route(lib, PEER_RING, same, 1, can, enabled) == (IPC_STAGED, DEFAULT_COPY)
            assert route(lib, DEVICE_STRIP_KIND, same, 1, can, enabled) == (DEVICE_STRIP, IN_PLACE)
            assert route(lib, DEVICE_STRIP_KIND, same, 0, can, enabled) == (DEVICE_STRIP, IN_PLACE)


def test_no_unknown_mapping_is_read_in_place(lib):
    """Whatever else is said of it, a peer ring with same_device = -1 goes through the strip and counts as IPC_STAGED:
    POLARIS_MERGE_IPC_UNKNOWN is no longer counted."""
    for kind, same, staged, can, enabled in itertools.product(range(4), (1, 0, -1), (0, 1), (1, 0, -1), (0, 1)):
        branch, rows = route(lib, kind, same, staged, can, enabled)
        assert branch != IPC_UNKNOWN
        if kind == PEER_RING and same == -1:
            assert (branch, rows) == (IPC_STAGED, DEFAULT_COPY)
