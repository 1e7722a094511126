"""The soft-decision CRC repair's kernels by themselves on the MI355X: tests/gpu/softfec_device_driver.hip links beside the
shipped gr_adsb_amd/csrc/adsb_softfec.hip and runs its launchers on guarded device buffers.  Every kernel-alone case of
tests/test_softfec.py runs unchanged (the driver has the emulator driver's entry points), so the device's bytes equal the
restatement's; one case of 4100 records takes the grid-stride loop through further rounds."""
import ctypes

import numpy as np
import pytest

import device_build
import softfec_cases as C
import softfec_replay as SR
import test_softfec as TS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sim():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    so = device_build.device_lib("adsb_softfec.hip", "softfec_device_driver.hip", "libadsb_softfec_device.so",
                                 ["adsb_softfec.h", "adsb_softfec_device.h", "adsb_reply_device.h", "adsb_env_hip.h"])
    return ctypes.CDLL(so)


cases = TS.cases


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("rule", sorted(C.RULES))
def test_records_kernel_equals_the_replay(sim, cases, rule, grid):
    TS.test_records_kernel_equals_the_replay(sim, cases, rule, grid)


def test_records_kernel_edges(sim, cases):
    TS.test_records_kernel_edges(sim, cases)


def test_records_kernel_at_ten_samples_per_microsecond(sim):
    TS.test_records_kernel_at_ten_samples_per_microsecond(sim)


@pytest.mark.parametrize("k", range(5))
def test_records_kernel_reads_every_input_format(sim, k):
    TS.test_records_kernel_reads_every_input_format(sim, k)


@pytest.mark.parametrize("rule", sorted(C.RULES))
def test_slices_kernel_equals_the_replay(sim, cases, rule):
    bits14, ok, tags = C.slices_of(np.resize(cases.records(), 40))
    want_bits, want_ok, want_rows = SR.replay_slices(bits14, ok, tags, cases.x, 2, C.RULES[rule])
    for grid in (1, 3):
        b, o = bits14.copy(), ok.copy()
        rows = np.full(len(ok), TS.FILL, dtype=np.uint8).repeat(8).view(SR.SOFT_DTYPE)
        rs = TS.rule_struct(C.RULES[rule])
        rc = sim.sim_soft_slices(TS._p(cases.x), ctypes.c_longlong(len(cases.x)), TS._p(tags), ctypes.c_int(2), ctypes.byref(rs), TS._p(b),
                                 TS._p(o), ctypes.c_int(len(ok)), TS._p(rows), ctypes.c_int(grid))
        assert rc == 0
        TS.same(b, want_bits), TS.same(o, want_ok), TS.same(rows, want_rows)


def test_many_records_take_further_grid_stride_rounds(sim, cases):
    """4100 records, 300 of them qualifying, on 256 workgroups (1024 wavefronts): five rounds of the loop, the last one ragged"""
    recs = cases.records()
    names = cases.names
    quiet = recs[names.index("clean")]
    qualifying = np.array([r for r, nm in zip(recs, names) if nm not in ("clean", "no_demod", "fec_df", "df20")], dtype=SR.REC_DTYPE)
    lst = np.full(4100, quiet, dtype=SR.REC_DTYPE)
    at = np.sort(np.random.default_rng(9).choice(4100, 300, replace=False))
    lst[at] = np.resize(qualifying, 300)
    want, rows = TS.check_records(sim, cases.x, len(cases.x), cases.x, lst, C.RULES["default"], 256)
    assert (rows["ncand"] > 0).sum() == 300 and (rows["nflip"] > 0).sum() >= 100
