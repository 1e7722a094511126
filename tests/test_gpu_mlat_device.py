"""adsb_stream_mlat's kernels on the MI355X itself, at the seams tests/test_mlat.py puts them to on the SIMT emulator: the shipped
translation unit gr_adsb_amd/csrc/adsb_mlat.hip, compiled with the library's flags, and its real launchers with their own
cover(), driven by tests/gpu/mlat_device_driver.hip -- the emulator driver's entry point sim_mlat on device memory, with the
same guard bytes, range checks and -ENOSPC rule (tests/sim/mlat_host_rule.h) and the same words of the carry (the emulator
driver's sim_mlat_carry).

(a) test_mlat.py's cases, imported unchanged, with this module's `sim`: what hipcc made of the ballots, shuffles and LDS
    staging against the replay, with test_mlat.TOL and compare()'s converge rule.  `grid` is ignored by the device driver, so
    those parametrisations run twice with equal effect.
(b) Every call of (a) with at most TWIN_MAX entries is repeated on the emulator library over the same arguments; the fixes, the
    member lists, the heads, the counts and the return code are compared as bytes, and
    test_the_device_equals_the_emulator_byte_for_byte, which runs last, asserts that none differed.  Both sides compile with
    -ffp-contract=off, the butterfly sums have a fixed order, and IEEE sqrt and / are correctly rounded on both.
(c) test_the_scan_with_more_than_256_chunks, imported too: k_mlat_scan's threads take two chunks each.
(d) test_the_second_grid_stride_round: 533 000 entries, more than 2048 workgroups' worth of range entries, heads and groups, so
    that every kernel's grid-stride loop goes round again under the real launchers; and the range arguments on that carry.
The expected rows of (c) and (d) are built by period: test_mlat.check_periodic."""
import ctypes
import os
import shutil
import subprocess
import tempfile
import time

import numpy as np
import pytest

import test_mlat as TM
from gr_adsb_amd import _native as N
from gr_adsb_amd import build as B
from test_mlat import (test_one_group_is_located, test_all_receivers_at_one_point_is_singular, test_a_hearing_one_second_off,      # noqa: F401
                       test_a_head_at_a_seam, test_tiles_of_foreign_entries_in_front_of_a_head, test_the_cap_of_64_candidates,
                       test_a_stream_heard_twice_and_a_stream_without_a_position, test_the_chain,
                       test_short_and_long_with_the_same_first_56_bits, test_the_range_is_half_open_and_min_rx,
                       test_no_space_states_the_counts_and_writes_nothing, test_an_empty_carry_and_a_carry_without_groups, test_icao,
                       test_random_fleets, test_the_scan_with_more_than_256_chunks)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV_DIR = os.path.join(HERE, "gpu")
DEV_SO = os.path.join(DEV_DIR, "libadsb_mlat_dev.so")
TWIN_MAX = 4096                   # entries: the largest carry of (a) is 2 * TILE + 14; the emulator takes seconds for (c), minutes for (d)
vp = ctypes.c_void_p


def device_lib():
    """adsb_mlat.hip with exactly the library's flags as one unit, the driver as a second, side by side; linked into DEV_SO"""
    mlat = os.path.join(B.CSRC, B.MLAT_SOURCE)
    drv = os.path.join(DEV_DIR, "mlat_device_driver.hip")
    srcs = [mlat, drv, os.path.join(HERE, "sim", "mlat_host_rule.h")] + [os.path.join(B.CSRC, f) for f in ("adsb_mlat.h", "adsb_mlat_device.h")]
    if not (os.path.exists(DEV_SO) and all(os.path.getmtime(DEV_SO) >= os.path.getmtime(s) for s in srcs)):
        t0 = time.time()
        compile_flags = [f for f in B.FLAGS if f != "-shared"]
        tmp = tempfile.mkdtemp(prefix="adsb_mlat_dev_")
        try:
            objs = [os.path.join(tmp, "adsb_mlat.o"), os.path.join(tmp, "driver.o")]
            cmds = [[B.hipcc()] + compile_flags + ["-c", mlat, "-o", objs[0]],
                    [B.hipcc()] + compile_flags + ["-Wall", "-Wextra", "-c", drv, "-o", objs[1]]]
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
    lib.sim_mlat_layout_bytes.restype = ctypes.c_ulonglong
    lib.sim_mlat_layout_bytes.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    return lib


@pytest.fixture(scope="module")
def emu():
    """the emulator library, or None where it cannot be built (no g++)"""
    if shutil.which("g++") is None:
        return None
    return TM.mlat_lib()


CARRY_FN = ctypes.CFUNCTYPE(None, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp)


@CARRY_FN
def numpy_carry(ts, bits, mk, stream, nc, zero_hash, out):
    """sim_mlat_carry where there is no emulator library: test_mlat.carry_words_numpy, held equal to it on the CPU"""
    arr = lambda p, ct, shape: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape)      # noqa: E731
    w = TM.carry_words_numpy(arr(ts, ctypes.c_double, (nc,)), arr(bits, ctypes.c_ubyte, (nc, 14)), arr(mk, ctypes.c_int, (nc,)),
                             arr(stream, ctypes.c_int, (nc,)), zero_hash)
    ctypes.memmove(out, w.ctypes.data, w.nbytes)


@pytest.fixture(scope="module")
def dev(emu):
    import torch                  # first, as _native.load() does: the library must bind to the HIP runtime torch bundles, or the
    assert torch.cuda.is_available(), "GPU tests need a GPU"      # process holds two runtimes and the later one finds no device
    lib = device_lib()
    assert lib.sim_mlat_fix_bytes() == N.MLAT_DTYPE.itemsize == 88
    lib.dev_mlat_set_carry(ctypes.cast(emu.sim_mlat_carry, vp) if emu is not None else numpy_carry)
    return lib


class Both:
    """sim_mlat of the device library; every call of at most TWIN_MAX entries is repeated on the emulator library with buffers
    of its own that start as the caller's did, and what differs as bytes is kept for the module's last test."""
    OUT = ((13, 14, 88), (16, 18, 4), (17, 18, 8), (20, 4, 4))      # (buffer, its length, bytes per item) among sim_mlat's arguments
    COUNTS = (15, 19, 21)

    def __init__(self, dev, emu):
        self.dev, self.emu, self.compared, self.differ = dev, emu, 0, []

    def sim_mlat(self, *a):
        nc = a[4].value
        size = [max(a[n].value, 1 if b == 20 else 0) * item for b, n, item in self.OUT]
        before = [ctypes.string_at(a[b], s) if s else b"" for (b, _, _), s in zip(self.OUT, size)]
        rc = self.dev.sim_mlat(*a)
        assert self.dev.dev_mlat_dead() == 0, "a HIP call failed (%d): no further GPU call is made" % rc
        if self.emu is None or nc > TWIN_MAX:
            return rc
        got = [ctypes.string_at(a[b], s) if s else b"" for (b, _, _), s in zip(self.OUT, size)]
        counts = [a[k]._obj.value for k in self.COUNTS]
        twin = list(a)
        bufs = [(ctypes.c_char * max(len(x), 1))() for x in before]
        for buf, x in zip(bufs, before):
            ctypes.memmove(buf, x, len(x))
        cnt = [ctypes.c_int(-1) for _ in self.COUNTS]
        for (b, _, _), buf in zip(self.OUT, bufs):
            twin[b] = buf
        for k, c in zip(self.COUNTS, cnt):
            twin[k] = ctypes.byref(c)
        rc2 = self.emu.sim_mlat(*twin)
        self.compared += 1
        if rc2 != rc or [c.value for c in cnt] != counts:
            self.differ.append(("rc / n_fixes / n_members / n_heads", nc, (rc, counts), (rc2, [c.value for c in cnt])))
        for name, g, buf, s in zip(("fixes", "member_stream", "member_ts", "heads"), got, bufs, size):
            if g != buf.raw[:s]:
                first = next(k for k in range(s) if g[k] != buf.raw[k])
                row = first // 88 if name == "fixes" else first
                self.differ.append((name, nc, "byte %d" % first,
                                    np.frombuffer(g, N.MLAT_DTYPE)[row] if name == "fixes" else g[first:first + 8],
                                    np.frombuffer(buf.raw[:s], N.MLAT_DTYPE)[row] if name == "fixes" else buf.raw[first:first + 8]))
        return rc

    def __getattr__(self, name):                      # the sizing exports
        return getattr(self.dev, name)


@pytest.fixture(scope="module")
def sim(dev, emu):
    return Both(dev, emu)


N_STRIDE = 8200 * TM.PERIOD       # 533 000 entries > 2048 * 256; 426 400 heads and 16 400 groups > 2048 * 4


def test_the_second_grid_stride_round(sim):
    """(d): one carry under the real launchers' cover(), which caps the grid at 2048 workgroups: k_mlat_heads, k_mlat_count and
    k_mlat_place go round again over the range's entries, k_mlat_groups over the heads, k_mlat_solve over the groups.  Then the
    range arguments on period boundaries: periods [a, b) of the same carry give exactly their slice of the full result."""
    assert N_STRIDE >= 2048 * 256 + 1
    fixes, ms, mt, heads, p0, per_f, per_m = TM.check_periodic(sim, "stride", N_STRIDE)
    print("stride: %d entries, %d heads, %d fixes, %d members" % (N_STRIDE, len(heads), len(fixes), len(ms)))
    assert len(heads) > 8192 and len(fixes) > 8192 and len(heads) // 4 > 2048 and len(fixes) // 4 > 2048
    arrays, _ = TM.periodic(N_STRIDE)
    per_h = len(heads) // (N_STRIDE // TM.PERIOD)
    a, b = 4001, 4011                                 # the range begins at entry 260 065: no multiple of 64
    rc, f2, ms2, mt2, heads2, nf, nm = TM.run_arrays(sim, *arrays, TM.RX8, t_lo=TM.EPOCH + a * TM.SPACING, t_hi=TM.EPOCH + b * TM.SPACING)
    assert rc == 0 and (nf, nm) == ((b - a) * per_f, (b - a) * per_m)
    want = fixes[a * per_f:b * per_f].copy()
    want["first"] -= a * per_m
    assert f2[:nf].tobytes() == want.tobytes()
    assert ms2[:nm].tobytes() == ms[a * per_m:b * per_m].tobytes() and mt2[:nm].tobytes() == mt[a * per_m:b * per_m].tobytes()
    assert np.array_equal(heads2, heads[a * per_h:b * per_h])


def test_the_device_equals_the_emulator_byte_for_byte(sim, emu):
    """(b), runs last in this file: of the calls above that both libraries took, none differed in a byte of the fixes, the
    member lists or the heads, in a count or in the return code."""
    if emu is None:
        pytest.skip("no g++ on this machine: the emulator library cannot be built, the device ran against the replay alone")
    assert sim.compared > 0, "the cases above ran"
    print("device = emulator over %d calls" % sim.compared)
    assert not sim.differ, (len(sim.differ), sim.differ[:3])
