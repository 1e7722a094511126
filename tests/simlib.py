"""ctypes wrapper around tests/sim/libadsb_sim.so (the device code run by the CPU SIMT emulator).
Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
SIM_SO = os.path.join(SIM_DIR, "libadsb_sim.so")


class SimOut(ctypes.Structure):
    _fields_ = [("n_rec", ctypes.c_int), ("n_kept", ctypes.c_int), ("overflow", ctypes.c_int),
                ("long_count", ctypes.c_int), ("flags", ctypes.c_uint), ("lastp", ctypes.c_longlong),
                ("last_kept", ctypes.c_longlong)]


REC_DTYPE = np.dtype([("offset", "<i8"), ("peak", "<f4"), ("median", "<f4"), ("bits", "u1", (14,)), ("flags", "<u2")])
assert REC_DTYPE.itemsize == 32


def build_sim(force=False):
    srcs = [os.path.join(SIM_DIR, "sim_driver.cpp"), os.path.join(SIM_DIR, "hipsim.h"),
            os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not force and os.path.exists(SIM_SO) and all(os.path.getmtime(SIM_SO) >= os.path.getmtime(s) for s in srcs):
        return SIM_SO
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                           srcs[0], "-o", SIM_SO])
    return SIM_SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_sim())
        _lib.sim_run.restype = ctypes.c_int
        _lib.sim_slice.restype = ctypes.c_int
    return _lib


def kernel_geometry():
    """(tile, forward halo, back halo) of k_detect's sliding LDS window, from the compiled device header."""
    t, f, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().sim_geometry(ctypes.byref(t), ctypes.byref(f), ctypes.byref(b))
    return t.value, f.value, b.value


def convert8(mode, iq8, scale):
    """body_convert<mode> (k_detect's in-register conversion) of interleaved 8-bit IQ -> float32 |IQ|^2; len(iq8) % 16 == 0."""
    raw = np.ascontiguousarray(iq8).view(np.uint32)
    out = np.empty(2 * len(raw), dtype=np.float32)
    lib().sim_convert8(ctypes.c_int(mode), raw.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(len(raw)),
                       ctypes.c_float(scale), out.ctypes.data_as(ctypes.c_void_p))
    return out


def sim_run(mode, data, sps, thr, in0_base, scan_lo, scan_hi, fall_hi, dem_hi, origin=0, prev_in0=0.0,
            end_is_call_end=1, prev_eob_stream=None, gate=True, grid_max=6, rec_cap=0, scale=1.0):
    """mode 0: complex64[n]; 1: float32 |IQ|^2 [n]; 2: int16 / 3: int8 / 4: uint8 interleaved IQ [2n]."""
    if mode >= 2:
        data = np.ascontiguousarray(data, dtype={2: np.int16, 3: np.int8, 4: np.uint8}[mode])
        n = len(data) // 2
    else:
        data = np.ascontiguousarray(data, dtype=np.complex64 if mode == 0 else np.float32)
        n = len(data)
    if prev_eob_stream is None:
        prev_eob_stream = origin + in0_base - 1
    cap = max(16, n // 2 + 16)
    out = np.zeros(cap, dtype=REC_DTYPE)
    so = SimOut()
    c = ctypes
    rc = lib().sim_run(c.c_int(mode), data.ctypes.data_as(c.c_void_p), c.c_longlong(n), c.c_longlong(in0_base),
                       c.c_longlong(scan_lo), c.c_longlong(scan_hi), c.c_longlong(fall_hi), c.c_longlong(dem_hi),
                       c.c_longlong(origin), c.c_float(thr), c.c_float(prev_in0), c.c_int(sps), c.c_int(end_is_call_end),
                       c.c_longlong(prev_eob_stream), c.c_int(1 if gate else 0), c.c_int(0), c.c_int(grid_max), c.c_int(rec_cap),
                       c.c_float(scale),
                       out.ctypes.data_as(c.c_void_p), c.c_int(cap), c.byref(so))
    assert rc == 0
    return out[:so.n_kept].copy(), so


def sim_canonical(mode, data, fs, thr, abs_offset=0, **kw):
    sps = int(fs // 1e6)
    H = 8 * sps
    n = len(data) // 2 if mode >= 2 else len(data)
    return sim_run(mode, data, sps, thr, in0_base=-(H - 1), scan_lo=-(H - 1), scan_hi=n - (H - 1), fall_hi=n - (H - 1),
                   dem_hi=n, origin=abs_offset, **kw)


def _call(fn, args, cap, gate=True):
    out = np.zeros(cap, dtype=REC_DTYPE)
    so = SimOut()
    rc = fn(*args, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(cap), ctypes.byref(so))
    assert rc == 0, rc
    return out[:so.n_kept].copy(), so


class SimFramer:
    """framer.work() through adsb_plan.h + the emulated kernels, state carried like the library does."""

    def __init__(self, fs, thr, grid_max=6):
        self.sps = int(fs // 1e6)
        self.thr = thr
        self.prev_in0 = ctypes.c_float(0.0)
        self.prev_eob = ctypes.c_longlong(-1)
        self.grid_max = grid_max

    def work(self, in0, N, nitems_written):
        c = ctypes
        in0 = np.ascontiguousarray(in0, dtype=np.float32)
        args = (in0.ctypes.data_as(c.c_void_p), c.c_longlong(len(in0)), c.c_longlong(N), c.c_longlong(nitems_written),
                c.c_float(self.thr), c.c_int(self.sps), c.byref(self.prev_in0), c.byref(self.prev_eob), c.c_int(self.grid_max))
        return _call(lib().sim_framer_work, args, max(16, len(in0) // 2 + 16))


def sim_shard(mode, data, origin, own_lo, own_hi, stream_len, fs, thr, head_cands=0, grid_max=6):
    c = ctypes
    data = np.ascontiguousarray(data, dtype=np.complex64 if mode == 0 else np.float32)
    args = (c.c_int(mode), data.ctypes.data_as(c.c_void_p), c.c_longlong(len(data)), c.c_longlong(origin),
            c.c_longlong(own_lo), c.c_longlong(own_hi), c.c_longlong(stream_len), c.c_float(thr), c.c_int(int(fs // 1e6)),
            c.c_int(head_cands), c.c_int(grid_max))
    return _call(lib().sim_shard, args, max(16, len(data) // 2 + 16), gate=False)


def sim_slice(in0, tag_idx, sps, want_ratio=True, fill=0):
    """k_slice over the tags; fill: the byte every output array holds before the kernel runs"""
    c = ctypes
    in0 = np.ascontiguousarray(in0, dtype=np.float32)
    tag_idx = np.ascontiguousarray(tag_idx, dtype=np.int64)
    nt = len(tag_idx)
    bits = np.full((nt, 14), fill, dtype=np.uint8)
    ok = np.full(nt, fill, dtype=np.uint8)
    ratio = np.full((nt, 112 * 4), fill, dtype=np.uint8).view(np.float32)
    lib().sim_slice(in0.ctypes.data_as(c.c_void_p), c.c_longlong(len(in0)), tag_idx.ctypes.data_as(c.c_void_p), c.c_int(nt),
                    c.c_int(sps), bits.ctypes.data_as(c.c_void_p), ok.ctypes.data_as(c.c_void_p),
                    ratio.ctypes.data_as(c.c_void_p) if want_ratio else None)
    return bits, ok, ratio


def unpack_bits(bits14):
    return np.unpackbits(np.asarray(bits14, dtype=np.uint8).reshape(-1, 14), axis=1, bitorder="big")


class tail_mode:
    """with simlib.tail_mode(1): ... -- 1 = always the tail kernel chain, 2 = always the one-workgroup fused tail
    (0 = the library's own choice by pass size)."""
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        lib().sim_set_tail_mode(self.mode)

    def __exit__(self, *a):
        lib().sim_set_tail_mode(0)


# the slicing sites of adsb_device.h (enum Route), logged by the emulator's ADSB_ROUTE
ROUTES = ("window", "pend", "pend_full", "flush", "long_fast", "long_clipped")


def route_reset():
    lib().sim_route_reset()


def route_offsets():
    """{route name: int64[] stream offsets of the bursts it sliced since route_reset(), in the order they were sliced}"""
    L = lib()
    L.sim_route_offsets.restype = ctypes.c_longlong
    assert L.sim_route_count() == len(ROUTES)
    out = {}
    for k, name in enumerate(ROUTES):
        n = L.sim_route_offsets(ctypes.c_int(k), None, ctypes.c_longlong(0))
        buf = np.zeros(max(n, 1), dtype=np.int64)
        L.sim_route_offsets(ctypes.c_int(k), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(n))
        out[name] = buf[:n]
    return out


class confidence_out:
    """with simlib.confidence_out(cap) as ratio: ... -- the runs inside also run k_confidence (ADSB_FLAG_CONFIDENCE) into
    ratio[cap][112] float32; row t belongs to kept record t of the LAST run, rows of records without a PDU are untouched.
    The array is filled with an all-ones bit pattern first."""
    def __init__(self, cap):
        self.buf = np.full((cap, 112), 0xFFFFFFFF, dtype=np.uint32).view(np.float32)

    def __enter__(self):
        lib().sim_set_confidence_out(self.buf.ctypes.data_as(ctypes.c_void_p))
        return self.buf

    def __exit__(self, *a):
        lib().sim_set_confidence_out(None)


class long_aware_gate:
    """with simlib.long_aware_gate(): ... -- the emulated device code runs with ADSB_FLAG_LONG_AWARE_GATE semantics."""
    def __enter__(self):
        lib().sim_set_long_aware(1)

    def __exit__(self, *a):
        lib().sim_set_long_aware(0)


# the turns of noise_median (adsb_device.h: enum MedianPath), logged by the emulator's ADSB_MEDIAN_PATH: bit k of a path word
MEDIAN_PATHS = ("hint_none", "hint_exact", "hint_below", "hint_above", "hint_refused",
                "one_16", "one_12", "one_8", "crowd_16", "crowd_12", "crowd_8", "bit_0",
                "upper_odd", "upper_exact_again", "upper_count", "upper_next")


class Units:
    """Single device functions on chosen inputs, through the entry points tests/sim/sim_driver.cpp and
    tests/gpu/detect_units_driver.hip share: Units(simlib.lib()) runs the emulator's twins of the device environment,
    Units(<the device driver's library>) the product's versions on the GPU."""

    def __init__(self, library, check=None):
        self.lib, self.check = library, check or (lambda: None)
        self.lib.sim_chips_match.restype = ctypes.c_int

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def noise_median(self, quant, windows, nwin, chain_start, hint0, want_paths=True):
        """-> (median bits, hint after each window, path word of each window or None)"""
        windows = np.ascontiguousarray(windows, dtype=np.float32)
        nwin, chain_start = np.ascontiguousarray(nwin, dtype=np.int32), np.ascontiguousarray(chain_start, dtype=np.int32)
        hint0 = np.ascontiguousarray(hint0, dtype=np.uint32)
        total = len(nwin)
        assert windows.shape == (total, 128) and chain_start[-1] == total and len(hint0) == len(chain_start) - 1
        med, hint = np.full(total, 0xDEADBEEF, dtype=np.uint32), np.full(total, 0xDEADBEEF, dtype=np.uint32)
        path = np.zeros(total, dtype=np.uint32) if want_paths else None
        self.lib.sim_noise_median(ctypes.c_int(1 if quant else 0), self._p(windows), self._p(nwin), self._p(chain_start),
                                  self._p(hint0), ctypes.c_int(len(hint0)), self._p(med), self._p(hint),
                                  self._p(path) if want_paths else None)
        self.check()
        return med, hint, path

    def chips_match(self, half, taps, raw=True):
        """half: 1, 2, 4, 10 = that instance of chips_match; -h = the run-time instance at h samples per chip.  raw=False: the
        instance for computed samples (taps without a signalling NaN)"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        assert taps.ndim == 2 and taps.shape[1] == 16
        out = np.full(len(taps), 0xEE, dtype=np.uint8)
        rc = self.lib.sim_chips_match(ctypes.c_int(half), ctypes.c_int(1 if raw else 0), self._p(taps), ctypes.c_int(len(taps)), self._p(out))
        self.check()
        assert rc == 0 and set(np.unique(out)) <= {0, 1}
        return out.astype(bool)

    def wave_min_max(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert rows.ndim == 2 and rows.shape[1] == 64
        mn, mx = np.full_like(rows, 0x5A5A5A5A), np.full_like(rows, 0x5A5A5A5A)
        self.lib.sim_wave_min_max(self._p(rows), ctypes.c_int(len(rows)), self._p(mn), self._p(mx))
        self.check()
        return mn, mx

    def wave_incl_scan(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert rows.ndim == 2 and rows.shape[1] == 64
        out = np.full_like(rows, 0x5A5A5A5A)
        self.lib.sim_wave_incl_scan(self._p(rows), ctypes.c_int(len(rows)), self._p(out))
        self.check()
        return out

    def lane_up1(self, rows, fill):
        rows, fill = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(fill, dtype=np.uint32)
        assert rows.ndim == 2 and rows.shape[1] == 64 and fill.shape == (len(rows),)
        out = np.full_like(rows, 0x5A5A5A5A)
        self.lib.sim_lane_up1(self._p(rows), self._p(fill), ctypes.c_int(len(rows)), self._p(out))
        self.check()
        return out

    def above4(self, acc, x, thr):
        """acc uint32[rows][64], x float32[rows][64][4], thr float32[rows] (one threshold per wavefront)"""
        acc, x = np.ascontiguousarray(acc, dtype=np.uint32), np.ascontiguousarray(x, dtype=np.float32)
        thr = np.ascontiguousarray(thr, dtype=np.float32)
        assert acc.shape == (len(thr), 64) and x.shape == (len(thr), 64, 4)
        out = np.full_like(acc, 0x5A5A5A5A)
        self.lib.sim_above4(self._p(acc), self._p(x), self._p(thr), ctypes.c_int(len(thr)), self._p(out))
        self.check()
        return out

    def bitrep32(self, x):
        x = np.ascontiguousarray(x, dtype=np.uint32)
        out = np.full(len(x), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        self.lib.sim_bitrep32(self._p(x), ctypes.c_int(len(x)), self._p(out))
        self.check()
        return out

    def mag2(self, x, y):
        x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == y.shape and x.ndim == 1
        out = np.full(len(x), 0x5A5A5A5A, dtype=np.uint32).view(np.float32)
        self.lib.sim_mag2(self._p(x), self._p(y), ctypes.c_longlong(len(x)), self._p(out))
        self.check()
        return out

    def convert8(self, mode, iq8, scale):
        """body_convert<mode> of interleaved 8-bit IQ -> float32 |IQ|^2; len(iq8) % 16 == 0"""
        raw = np.ascontiguousarray(iq8).view(np.uint32)
        out = np.full(2 * len(raw), 0x5A5A5A5A, dtype=np.uint32).view(np.float32)
        self.lib.sim_convert8(ctypes.c_int(mode), self._p(raw), ctypes.c_longlong(len(raw)), ctypes.c_float(scale), self._p(out))
        self.check()
        return out
