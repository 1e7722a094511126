"""The de-duplication step's kernels on the MI355X itself, at the seams tests/test_dedup.py puts them to on the SIMT emulator: the
shipped translation unit gr_adsb_amd/csrc/adsb_dedup.hip, compiled with the library's flags, and its real launchers with their
own cover(), driven by tests/gpu/dedup_device_driver.hip -- the emulator driver's entry point sim_dedup_step on device memory,
every array a part of its own with a guard tail, every part read back whole behind every launcher.

(a) test_dedup.py's section "the kernels alone" (test_dedup.ALONE), imported unchanged, with this module's `sim`: what hipcc
    made of k_dedup_find's LDS tiles, its block-uniform loops and the binary searches against the plain statement of every
    output byte.  `grid` is ignored by the device driver, so each case runs twice with equal effect.
(c) test_the_second_grid_stride_round: one step of 526 500 records against a carry of 4 160 entries, built by period
    (test_dedup.periodic_step), so that k_dedup_entries, k_dedup_find, k_dedup_merge and k_dedup_mark all go round their
    grid-stride loops a second time under cover()'s cap of 2048 workgroups.
Every output is an integer or a bit pattern and the statements give every byte: there is no tolerance and no comparison with
the emulator's bytes."""
import ctypes

import pytest

import device_build
import test_dedup as TD
from test_dedup import (test_alone_one_reply_heard_by_many_streams, test_alone_the_earliest_match_lies_in_a_later_partial_tile,      # noqa: F401
                        test_alone_more_than_two_tiles_of_hearings, test_alone_a_carry_range_on_both_sides_in_time,
                        test_alone_all_timestamps_equal, test_alone_window_zero, test_alone_records_with_marker_zero,
                        test_alone_the_merge_and_the_cut, test_alone_items)

pytestmark = pytest.mark.gpu

COVER_CAP = 2048 * 256            # threads of the largest grid cover() gives
PERIODS = 8100                    # 526 500 records
HORIZON = 100.0
ran = {"imported": 0, "calls": 0}


class Device:
    """sim_dedup_step of the device library; after every call the library must still be alive"""

    def __init__(self, lib):
        self.lib = lib

    def sim_dedup_step(self, *a):
        rc = self.lib.sim_dedup_step(*a)
        ran["calls"] += 1
        assert self.lib.dev_dedup_dead() == 0, "a HIP call failed (%d): no further GPU call is made" % rc
        return rc


@pytest.fixture(scope="module")
def sim():
    import torch                  # first, as _native.load() does: the library must bind to the HIP runtime torch bundles, or the
    assert torch.cuda.is_available(), "GPU tests need a GPU"      # process holds two runtimes and the later one finds no device
    so = device_build.device_lib("adsb_dedup.hip", "dedup_device_driver.hip", "libadsb_dedup_dev.so", ("adsb_dedup.h", "adsb_dedup_device.h"))
    return Device(ctypes.CDLL(so))


@pytest.fixture(autouse=True)
def count_imported(request):
    yield
    ran["imported"] += request.function.__module__ == "test_dedup"


def test_the_imports_are_the_whole_section():
    assert sorted(TD.ALONE) == sorted(k for k, v in globals().items() if k.startswith("test_alone_") and v.__module__ == "test_dedup")


def test_the_second_grid_stride_round(sim):
    """(c): every kernel's work exceeds the largest grid, from the sizes alone; then every output byte against the statement
    built by period."""
    w, d_alone, d_carry = TD.periodic_step(PERIODS, HORIZON)
    assert w.n > COVER_CAP and w.nc + w.n > COVER_CAP and w.nc >= 4096      # entries, find and mark stride over n, the merge over nc + n
    assert 0 < w.exp_state["off"][0] < w.n and (w.exp_dup == -2).sum() == (d_carry == -2).sum() * (w.nc // TD.P_PERIOD)
    print("stride: %d records against a carry of %d entries, %d duplicates, the cut at %d" %
          (w.n, w.nc, (w.exp_dup != -1).sum(), w.exp_state["off"][0]))
    w.check(sim, grids=(1,))


def test_the_imported_cases_ran():
    """runs last in this file: says how many of test_dedup.py's cases ran on the device, through how many steps"""
    print("device: %d imported cases, %d calls of sim_dedup_step" % (ran["imported"], ran["calls"]))
    assert ran["calls"] > ran["imported"] > 0
