"""CPU test of k_shade_wave's automatic grid (polaris_amd/csrc/trace_plan.h, shade_wave_grid with option shade_wgs_per_cu = 0).

The grid follows the kernel's residency -- TraceScene::shade_wave_resident, which the library asks of the occupancy API; the checker's
scene keeps the header's default of 5 workgroups (20 waves) per CU -- and gives every wave the same number of groups: with `waves` = 4
x CUs x resident and `rounds` = ceil(groups / waves), it is ceil(groups / (4 x rounds)) workgroups.  Every expectation is worked out
by hand from that rule; none is read back from the library.  (tests/test_trace_plan_cpu.py pins the grid of an explicit
shade_wgs_per_cu, which is taken as given.)
"""
from test_trace_plan_cpu import grids, lib  # noqa: F401  (the fixture that builds tests/tools/trace_plan_check.cpp)

AUTO = dict(shade_wgs_per_cu=0)   # 256 CUs x 5 workgroups x 4 waves = 5120 resident waves


def test_up_to_the_resident_waves_every_wave_takes_one_group(lib):
    assert grids(lib, 1, **AUTO)[2] == 1
    assert grids(lib, 9, **AUTO)[2] == 1                 # 2 groups
    assert grids(lib, 33, **AUTO)[2] == 2                # 5 groups
    assert grids(lib, 8 * 4096, **AUTO)[2] == 1024       # 4096 groups: four workgroups per CU
    assert grids(lib, 8 * 5117, **AUTO)[2] == 1280       # 5117 groups round up to ...
    assert grids(lib, 8 * 5120, **AUTO)[2] == 1280       # ... all the GPU holds: five per CU


def test_beyond_them_the_fewest_workgroups_of_equal_shares(lib):
    assert grids(lib, 8 * 5121, **AUTO)[2] == 641        # two rounds: ceil(5121 / 8)
    assert grids(lib, 8 * 8192, **AUTO)[2] == 1024       # the headline frame's launches: two groups for each of 4096 waves
    assert grids(lib, 8 * 10240, **AUTO)[2] == 1280      # two rounds on every resident wave
    assert grids(lib, 8 * 10241, **AUTO)[2] == 854       # three rounds: ceil(10241 / 12)
    assert grids(lib, 8 * 16384, **AUTO)[2] == 1024      # four rounds (ceil(16384 / 5120)): 16384 / 16
    assert grids(lib, 8 * 8192 - 7, **AUTO)[2] == 1024   # a started group counts


def test_it_scales_with_the_compute_units_and_never_exceeds_what_they_hold(lib):
    assert grids(lib, 8 * 8192, num_cus=64, **AUTO)[2] == 293     # 1280 waves: 7 rounds, ceil(8192 / 28)
    assert grids(lib, 8 * 8192, num_cus=304, **AUTO)[2] == 1024   # 6080 waves: 2 rounds
    for cus in (64, 256, 304):
        for groups in (1, 7, 1279, 1281, 5119, 5121, 6079, 6081, 8192, 100000):
            g = grids(lib, 8 * groups, num_cus=cus, **AUTO)[2]
            waves = 4 * cus * 5
            rounds = -(-groups // waves)
            assert 1 <= g <= 5 * cus and 4 * g * rounds >= groups, (cus, groups, g)   # resident at once, and enough for every group
            assert g == 1 or 4 * (g - 1) * rounds < groups, (cus, groups, g)            # ... and no more than that takes


def test_an_explicit_option_is_taken_as_given(lib):
    assert grids(lib, 8 * 8192, shade_wgs_per_cu=5)[2] == 1280
    assert grids(lib, 8 * 8192, shade_wgs_per_cu=8)[2] == 2048
    assert grids(lib, 8 * 8192, shade_wgs_per_cu=16)[2] == 2048   # never more workgroups than groups for their waves
