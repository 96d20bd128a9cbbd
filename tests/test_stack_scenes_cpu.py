"""CPU proof that the scenes of tests/tools/stack_scenes.py sit on the traversal stack's boundaries and that their rays reach the
deep end -- the preconditions of tests/test_gpu_stack_depth.py, counted here so that the GPU comparison cannot pass vacuously.

* the layout's max_stack (scene_layout.h: need + 1) equals the case's S exactly; S = 33 is refused with the stack-need message;
* per case and per walk the case is meant for (closest hit and any hit nearer-first; any hit in stored order for the mirrored
  scenes), at least 32 rays hold EXACTLY the most the layout allows -- S - 1 entries with several instances, S - 2 in a scene that is
  one instance -- and none holds more (tests/tools/layout_check.cpp layout_check_high_water, the kernels' rules on the CPU);
* `retry`: max_leaf_tris = 1 alone makes build_layout answer "@retry-without-subdivision"; with the fallback the layout is the
  unsplit one;
* the oracle's closest-hit rate lies strictly between 0.2 and 1 and its any-hit answers differ (what test_gpu_ties.Want asks).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from polaris_amd import ctypes_api as T
from test_scene_layout import harness, traverse  # noqa: F401  (the fixture that builds tests/tools/layout_check.cpp)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import stack_scenes as SS  # noqa: E402

NO_RETRY = 0x100


def high_water(lib, sc, rays, order, max_leaf=0):
    """-> (entries (n,) int32, counters (7,) uint64, "") or (None, None, error text)."""
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.zeros(len(rays), np.int32)
    cnt = np.zeros(7, np.uint64)
    err = C.create_string_buffer(256)
    view = T.scene_view(sc)
    fn = lib.layout_check_high_water
    fn.argtypes = [C.POINTER(T.SceneView), C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    rc = fn(C.byref(view), max_leaf, rays.ctypes.data, len(rays), order, out.ctypes.data, cnt.ctypes.data, err, 256)
    return (out, cnt, "") if rc == 0 else (None, None, err.value.decode())


@pytest.mark.parametrize("tag", SS.TRACED)
def test_exact_stack_need_and_rays_at_the_high_water_mark(harness, oracle, tag):  # noqa: F811
    sc, rays = SS.case(tag)
    c = SS.CASES[tag]
    assert rays.shape == (512, 8)
    want = SS.held(tag)
    for order in (0, 1, 2):
        entries, cnt, err = high_water(harness, sc, rays, order)
        assert err == "", err
        assert int(cnt[5]) == c["S"], (tag, "max_stack", int(cnt[5]))
        assert entries.max() <= want, (tag, order, int(entries.max()))               # the layout's bound holds in every walk
        at_mark = int((entries == want).sum())
        print(f"{tag}: S = {c['S']}, order {order}: {at_mark} rays hold {want} entries (deepest: {int(entries.max())})")
        if order in SS.orders(tag):
            assert at_mark >= 32, (tag, order, at_mark, int(entries.max()), want)
    # the oracle on these rays: neither all hit nor nearly all missed; and the kernels' rules on the CPU agree with it
    hit, wuvt, it = oracle.intersect(sc, rays)
    occ, _, _ = oracle.intersect(sc, rays, any_hit=True)
    assert 0.2 < (hit != 0).mean() < 1.0, (tag, float((hit != 0).mean()))
    assert 0 < (occ != 0).sum() < len(rays)
    if c["family"] == "instanced":   # some rays leave the chain instance with nothing hit and meet a decoy under the restored world-space ray
        assert 0 < (it[hit != 0, 0] != SS.DECOYS).sum() < (hit != 0).sum(), tag
    got, _ = traverse(harness, sc, rays, 0)
    h = hit != 0
    assert np.array_equal(got[:, 5] != 0, h)
    assert np.array_equal(got[h][:, [1, 0]], it[h]) and np.array_equal(got[h][:, 2], wuvt[h][:, 3].view(np.int32))
    assert np.array_equal(traverse(harness, sc, rays, 0, any_hit=True)[0][:, 5] != 0, occ != 0)


@pytest.mark.parametrize("tag", SS.REFUSED)
def test_a_need_of_33_entries_is_refused(harness, tag):  # noqa: F811
    sc, rays = SS.case(tag)
    for max_leaf in (0, 1):
        entries, _, err = high_water(harness, sc, rays[:1], 0, max_leaf)
        assert entries is None and "BVH needs a traversal stack of 33 entries" in err, (tag, err)


def test_retry_falls_back_to_the_unsplit_tree(harness):  # noqa: F811
    sc, rays = SS.case("retry")
    _, plain, err = high_water(harness, sc, rays, 0, 0)
    assert err == "" and int(plain[5]) == 32
    entries, _, err = high_water(harness, sc, rays[:1], 0 | NO_RETRY, 1)
    assert entries is None and err == "@retry-without-subdivision", err              # subdividing the 12-triangle leaf needs more than 32
    _, split, err = high_water(harness, sc, rays, 0, 1)
    assert err == "" and [int(v) for v in split[3:6]] == [int(v) for v in plain[3:6]]  # same pair records, slots and max_stack
    # (a leaf size that leaves the twelve together changes nothing and needs no retry)
    _, kept, err = high_water(harness, sc, rays[:1], 0 | NO_RETRY, 12)
    assert err == "" and [int(v) for v in kept[3:6]] == [int(v) for v in plain[3:6]]


def test_the_moved_nested_shells_scene_keeps_its_layout(harness):  # noqa: F811
    """tests/test_gpu_parity.py and test_gpu_kernel_selection.py pin the 24-entry variant on it: max_stack = n + 2."""
    for n, want in ((14, 16), (22, 24), (30, 32)):
        _, cnt, err = high_water(harness, SS._nested_shells_scene(n), np.zeros((0, 8), np.float32), 0)
        assert err == "" and int(cnt[5]) == want
    assert "33 entries" in high_water(harness, SS._nested_shells_scene(31), np.zeros((0, 8), np.float32), 0)[2]
