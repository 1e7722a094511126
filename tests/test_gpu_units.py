"""noise_median, chips_match, body_convert and the device environment's primitives on the MI355X itself, one function at a time:
tests/gpu/detect_units_driver.hip includes the product's gr_adsb_amd/csrc/adsb_env_hip.h (inline assembly, DPP) and adsb_device.h,
is compiled with the library's flags, and has the entry points of the emulator driver on device memory.

(a) noise_median: the arrays of tests/median_cases.py, both instances; bits equal to median_cases.median_ref, the carried hint
    equal to the reference's lower-middle key, and both byte-equal to the emulator's where g++ exists.
(b) tests/test_units.py's cases, imported unchanged, with this module's `units`: the product's versions of the primitives and
    what hipcc made of chips_match against the NumPy definitions that hold the emulator's twins on the CPU.
(c) k_unit_convert<3|4|5|6>: every byte pair at every scale of test_conversion_exact.SCALES against ref_iq8, bit for bit.
After every call: no HIP error, and the guard words behind every output buffer untouched."""
import ctypes
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import edge_cases as E
import median_cases as M
import simlib
import test_conversion_exact as TC
from gr_adsb_amd import build as B
from test_units import (test_wave_min_max, test_wave_incl_scan, test_lane_up1, test_bitrep32, test_above4, test_mag2,      # noqa: F401
                        test_chips_match_every_pattern, test_chips_match_edges)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV_DIR = os.path.join(HERE, "gpu")
DEV_SO = os.path.join(DEV_DIR, "libadsb_units_dev.so")


def device_lib():
    """the driver, one translation unit, with exactly the library's flags plus -Wall -Wextra"""
    drv = os.path.join(DEV_DIR, "detect_units_driver.hip")
    srcs = [drv] + [os.path.join(B.CSRC, f) for f in ("adsb_env_hip.h", "adsb_device.h")]
    if not (os.path.exists(DEV_SO) and all(os.path.getmtime(DEV_SO) >= os.path.getmtime(s) for s in srcs)):
        t0 = time.time()
        cmd = [B.hipcc()] + B.FLAGS + ["-Wall", "-Wextra", drv, "-o", DEV_SO]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (cmd, r.stdout)
        print("built %s in %.1f s" % (os.path.relpath(DEV_SO, HERE), time.time() - t0))
    return ctypes.CDLL(DEV_SO)


@pytest.fixture(scope="module")
def units():
    import torch                  # first, as _native.load() does: the library must bind to the HIP runtime torch bundles
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = device_lib()
    lib.dev_units_guard_bad.restype = ctypes.c_longlong

    def check():
        assert lib.dev_units_dead() == 0, "a HIP call failed (%d): no further GPU call is made" % lib.dev_units_dead()
        assert lib.dev_units_guard_bad() == 0, "%d guard words behind an output buffer were written" % lib.dev_units_guard_bad()

    assert lib.sim_median_path_count() == len(M.PATHS)
    return simlib.Units(lib, check)


@pytest.fixture(scope="module")
def emu():
    """the emulator library, or None where it cannot be built (no g++)"""
    if shutil.which("g++") is None:
        return None
    return simlib.Units(simlib.lib())


def where(chains, start, b):
    return chains[int(np.searchsorted(start, b, side="right")) - 1].name


@pytest.mark.parametrize("quant", [False, True], ids=["float", "quant"])
def test_noise_median_equals_the_reference(units, emu, quant):
    """(a).  The device's median bits and carried hints, the reference's, and the emulator's, printed before they are compared."""
    chains, packed, (med, key, _) = M.all_chains(quant)
    windows, nwin, start, hint0 = packed
    got_med, got_hint, _ = units.noise_median(quant, *packed, want_paths=False)
    bad = np.flatnonzero(got_med != med)
    for b in bad[:20]:
        print("median differs: %s window %d, n %d: device %08x reference %08x" % (where(chains, start, b), b, nwin[b], got_med[b], med[b]))
    badh = np.flatnonzero(got_hint != key)
    for b in badh[:20]:
        print("hint differs: %s window %d, n %d: device %08x reference %08x" % (where(chains, start, b), b, nwin[b], got_hint[b], key[b]))
    print("%d windows in %d chains: %d medians, %d hints differ from the reference" % (len(med), len(chains), len(bad), len(badh)))
    assert len(bad) == 0 and len(badh) == 0
    if emu is not None:
        e_med, e_hint, _ = emu.noise_median(quant, *packed)
        assert got_med.tobytes() == e_med.tobytes() and got_hint.tobytes() == e_hint.tobytes()


def test_noise_median_writes_only_its_windows(units):
    """a grid-stride round with more chains than 4 * 1024 wavefronts, chains of no window among them; med_out / hint_out of a
    window are written once and nothing else is"""
    rng = np.random.default_rng(5)
    n_chains = 4 * 1024 + 37
    lens = rng.integers(0, 3, n_chains)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    total = int(start[-1])
    windows = np.zeros((total, M.WIN), dtype=np.float32)
    nwin = rng.integers(0, 101, total).astype(np.int32)
    ws = []
    for k in range(total):
        w = rng.exponential(1.0, nwin[k]).astype(np.float32)
        windows[k, :nwin[k]] = w
        ws.append(w)
    med, hint, _ = units.noise_median(False, windows, nwin, start, np.zeros(n_chains, dtype=np.uint32), want_paths=False)
    ref = [M.median_ref(w) for w in ws]
    assert np.array_equal(med, np.array([r[0] for r in ref], dtype=np.uint32))
    assert np.array_equal(hint, np.array([r[1] for r in ref], dtype=np.uint32))


@pytest.mark.parametrize("scale", TC.SCALES)
def test_body_convert_every_pair(units, scale):
    """(c): k_detect's in-register conversion of 16-byte loads; modes 5 and 6 (the dot-product instances) wherever the library
    would choose them"""
    for mode, dtype, ob in ((3, np.int8, False), (4, np.uint8, True)):
        b = TC.every_pair(dtype)
        want = TC.ref_iq8(b, scale, ob)
        TC.assert_bits(units.convert8(mode, b, scale), want, "body_convert<%d>, scale %r" % (mode, scale))
        if E.is_pow2(scale):
            TC.assert_bits(units.convert8(mode + 2, b, scale), want, "body_convert<%d>, scale %r" % (mode + 2, scale))
