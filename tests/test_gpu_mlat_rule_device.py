"""adsb_stream_mlat_rule's kernels on the MI355X itself, at the cases tests/test_mlat_rule.py puts them to on the SIMT emulator:
the shipped translation units gr_adsb_amd/csrc/adsb_mlat.hip and adsb_mlat_rule.hip, compiled with the library's flags, and
their real launchers with their own cover(), driven by tests/gpu/mlat_rule_device_driver.hip -- the emulator driver's entry
point sim_mlat_rule on device memory, with the same guard bytes, argument table, range checks and -ENOSPC rule
(tests/sim/mlat_rule_host_rule.h) and the same words of the carry.

(a) test_mlat_rule.py's cases, imported unchanged, with this module's `sim`: what hipcc made of the damped solve against the
    replay, with test_mlat_rule.TOL and compare()'s rule.
(b) Every damped call of (a) with at most TWIN_MAX entries is repeated on the emulator library over the same arguments; the
    fixes, the aux rows, the member lists, the heads, the counts and the return code are compared as bytes, doubles included,
    and test_the_device_equals_the_emulator_byte_for_byte, which runs last, asserts that none differed.  Both sides compile
    with -ffp-contract=off, the butterfly sums have a fixed order, the height uses sqrt and / only, and IEEE sqrt and / are
    correctly rounded on both.
(c) test_the_second_grid_stride_round: 2 750 periods of test_mlat_rule.py's periodic carry, 41 250 entries with 13 750 heads and
    8 250 groups -- more than 2048 workgroups of four wavefronts' worth of each, so that k_mlat_groups_rule and k_mlat_solve_lm go
    round their grid-stride loops again under the real launchers; the smallest such carry but for the margin of 58 groups."""
import ctypes
import os
import shutil
import subprocess
import tempfile
import time

import numpy as np
import pytest

import test_mlat as TM
import test_mlat_rule as TR
from gr_adsb_amd import _native as N
from gr_adsb_amd import build as B
from test_mlat_rule import (test_gauss_newton_through_the_rule_is_adsb_stream_mlat, test_one_group_is_located, test_the_number_of_hearings,      # noqa: F401
                            test_aided_groups, test_three_hearings_beside_four, test_altitude_formats,
                            test_all_receivers_at_one_point_is_singular, test_the_restart, test_the_argument_table,
                            test_the_damped_rule_converges_where_the_undamped_one_does, test_a_periodic_carry)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV_DIR = os.path.join(HERE, "gpu")
DEV_SO = os.path.join(DEV_DIR, "libadsb_mlat_rule_dev.so")
TWIN_MAX = 4096
vp = ctypes.c_void_p


def device_lib():
    """adsb_mlat.hip and adsb_mlat_rule.hip with exactly the library's flags, a unit each, and the driver; linked into DEV_SO"""
    units = [os.path.join(B.CSRC, B.MLAT_SOURCE), os.path.join(B.CSRC, B.MLAT_RULE_SOURCE), os.path.join(DEV_DIR, "mlat_rule_device_driver.hip")]
    srcs = units + [os.path.join(DEV_DIR, "mlat_device_driver.hip"), os.path.join(HERE, "sim", "mlat_host_rule.h"),
                    os.path.join(HERE, "sim", "mlat_rule_host_rule.h")] + \
        [os.path.join(B.CSRC, f) for f in ("adsb_mlat.h", "adsb_mlat_device.h", "adsb_mlat_rule.h", "adsb_mlat_rule_device.h")]
    if not (os.path.exists(DEV_SO) and all(os.path.getmtime(DEV_SO) >= os.path.getmtime(s) for s in srcs)):
        t0 = time.time()
        compile_flags = [f for f in B.FLAGS if f != "-shared"]
        tmp = tempfile.mkdtemp(prefix="adsb_mlat_rule_dev_")
        try:
            objs = [os.path.join(tmp, "unit%d.o" % k) for k in range(len(units))]
            cmds = [[B.hipcc()] + compile_flags + (["-Wall", "-Wextra"] if k == 2 else []) + ["-c", u, "-o", o] for k, (u, o) in enumerate(zip(units, objs))]
            jobs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for c in cmds]
            for c, p in zip(cmds, jobs):
                text = p.communicate()[0]
                assert p.returncode == 0, (c, text)
                if text.strip():
                    print(text)
            subprocess.check_call([B.hipcc()] + B.FLAGS + objs + ["-o", DEV_SO])
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print("built %s in %.1f s" % (os.path.relpath(DEV_SO, HERE), time.time() - t0))
    lib = ctypes.CDLL(DEV_SO)
    for f in (lib.sim_mlat_layout_bytes, lib.sim_mlat_rule_layout_bytes):
        f.restype = ctypes.c_ulonglong
        f.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    return lib


@pytest.fixture(scope="module")
def emu():
    """the emulator library: the twin of (b), and the carry's words"""
    assert shutil.which("g++") is not None, "the emulator library is this file's other half: it needs g++"
    return TR.rule_lib()


@pytest.fixture(scope="module")
def dev(emu):
    import torch                  # first, as _native.load() does: the library must bind to the HIP runtime torch bundles
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = device_lib()
    assert lib.sim_mlat_fix_bytes() == N.MLAT_DTYPE.itemsize == 88 and lib.sim_mlat_aux_bytes() == N.MLAT_AUX_DTYPE.itemsize == 32
    lib.dev_mlat_set_carry(ctypes.cast(emu.sim_mlat_carry, vp))
    return lib


class Both:
    """sim_mlat_rule of the device library; every call of at most TWIN_MAX entries is repeated on the emulator library with
    buffers of its own that start as the caller's did, and what differs as bytes is kept for the module's last test.  sim_mlat
    (what _GN is compared with) is the device library's; sim_mlat_alt_ft, the device function called on the host, exists on the
    emulator's side only -- the device's alt_ft comes back in the aux rows."""
    COUNTS = (20, 24, 26)
    NAMES = ("fixes", "aux", "member_stream", "member_ts", "heads")

    def __init__(self, dev, emu):
        self.dev, self.emu, self.compared, self.differ = dev, emu, 0, []
        self.sim_mlat_alt_ft = emu.sim_mlat_alt_ft

    def sim_mlat(self, *a):
        rc = self.dev.sim_mlat(*a)
        assert self.dev.dev_mlat_dead() == 0, "a HIP call failed (%d): no further GPU call is made" % rc
        return rc

    def sim_mlat_rule(self, *a):
        nc, cap, member_cap = a[4].value, a[19].value, a[23].value
        out = [(17, cap * 88), (18, cap * 32 if a[18].value else 0), (21, member_cap * 4), (22, member_cap * 8), (25, max(nc, 1) * 4)]
        before = [ctypes.string_at(a[b], s) if s else b"" for b, s in out]
        rc = self.dev.sim_mlat_rule(*a)
        assert self.dev.dev_mlat_dead() == 0, "a HIP call failed (%d): no further GPU call is made" % rc
        if nc > TWIN_MAX:
            return rc
        got = [ctypes.string_at(a[b], s) if s else b"" for b, s in out]
        counts = [a[k]._obj.value for k in self.COUNTS]
        twin = list(a)
        bufs = [ctypes.create_string_buffer(x, max(len(x), 1)) for x in before]
        cnt = [ctypes.c_int(-1) for _ in self.COUNTS]
        for (b, s), buf in zip(out, bufs):
            if s or b != 18:
                twin[b] = buf
        for k, c in zip(self.COUNTS, cnt):
            twin[k] = ctypes.byref(c)
        rc2 = self.emu.sim_mlat_rule(*twin)
        self.compared += 1
        if rc2 != rc or [c.value for c in cnt] != counts:
            self.differ.append(("rc / n_fixes / n_members / n_heads", nc, (rc, counts), (rc2, [c.value for c in cnt])))
        for name, g, buf, (b, s) in zip(self.NAMES, got, bufs, out):
            if g != buf.raw[:s]:
                first = next(k for k in range(s) if g[k] != buf.raw[k])
                self.differ.append((name, nc, "byte %d" % first, g[first - first % 8:first - first % 8 + 8], buf.raw[first - first % 8:first - first % 8 + 8]))
        return rc

    def __getattr__(self, name):                      # the sizing exports
        return getattr(self.dev, name)


@pytest.fixture(scope="module")
def sim(dev, emu):
    return Both(dev, emu)


N_PERIODS = 2750


def test_the_second_grid_stride_round(sim):
    """(c): one periodic carry under the real launchers' cover(), which caps the grid at 2048 workgroups of four wavefronts:
    k_mlat_groups_rule goes round again over the heads, k_mlat_solve_lm over the groups.  Period 0 is the emulator's bytes (its own
    call, twinned); every period is period 0 bit for bit."""
    fixes, aux, heads = TR.check_periodic(sim, "stride", N_PERIODS)
    print("stride: %d entries, %d heads, %d fixes" % (N_PERIODS * TR.PERIOD, len(heads), len(fixes)))
    assert len(heads) > 2048 * 4 and 2048 * 4 < len(fixes) < 2048 * 4 + 64


def test_the_device_equals_the_emulator_byte_for_byte(sim):
    """(b), runs last in this file: of the calls above that both libraries took, none differed in a byte of the fixes, the aux
    rows, the member lists or the heads, in a count or in the return code."""
    assert sim.compared > 0, "the cases above ran"
    print("device = emulator over %d calls" % sim.compared)
    assert not sim.differ, (len(sim.differ), sim.differ[:3])
