"""The device environment's primitives and chips_match by themselves, each against a definition written in NumPy here.

adsb_device.h is written against a small environment -- adsb_above4, adsb_mag2, adsb_fmax3, adsb_lane_up1, adsb_wave_incl_scan,
adsb_wave_min_u32 / _max_u32, adsb_bitrep32, ... -- that exists twice: the product's versions with inline assembly and DPP
(gr_adsb_amd/csrc/adsb_env_hip.h) and the SIMT emulator's plain C++ twins (tests/sim/hipsim.h).  The tests below take a `units`
fixture: here it is the emulator library, so they hold the TWINS to the definitions; tests/test_gpu_units.py imports the same
functions with the device driver's library, so the MI355X runs the product's versions against the very same definitions."""
import numpy as np
import pytest

import simlib
import test_conversion_exact as TC

F32 = np.float32
QNAN, SNAN = 0x7FC00000, 0x7FA00000


def f32(bits):
    return np.asarray(bits, dtype=np.uint64).astype(np.uint32).view(F32)


@pytest.fixture(scope="module")
def units():
    return simlib.Units(simlib.lib())


# ---- wave minimum / maximum ---------------------------------------------------------------------------------------------------
def test_wave_min_max(units):
    rng = np.random.default_rng(124)
    rows = [rng.integers(0, 1 << 32, 64) for _ in range(64)]
    for lane in range(64):                                   # the extreme value at each lane in turn
        lo = rng.integers(1000, 1 << 31, 64)
        lo[lane] = 3
        hi = rng.integers(1000, 1 << 31, 64)
        hi[lane] = 0xFFFFFFF0
        edge = np.full(64, 0xFFFFFFFF)                       # ... among the fill values themselves
        edge[lane] = 0xFFFFFFFE
        zero = np.zeros(64, dtype=np.int64)
        zero[lane] = 1
        rows += [lo, hi, edge, zero]
    rows += [np.full(64, 0xFFFFFFFF), np.zeros(64, dtype=np.int64), np.arange(64), np.arange(64)[::-1] + 5]
    rows = np.array(rows, dtype=np.uint32)
    mn, mx = units.wave_min_max(rows)
    assert np.array_equal(mn, np.repeat(rows.min(axis=1)[:, None], 64, axis=1))      # read in every lane
    assert np.array_equal(mx, np.repeat(rows.max(axis=1)[:, None], 64, axis=1))


# ---- inclusive scan -----------------------------------------------------------------------------------------------------------
def test_wave_incl_scan(units):
    rng = np.random.default_rng(114)
    rows = [np.ones(64, dtype=np.int64), np.full(64, 0xFFFFFFFF), np.zeros(64, dtype=np.int64)]
    for lane in range(64):
        r = np.zeros(64, dtype=np.int64)
        r[lane] = 1
        rows.append(r)
    rows += [rng.integers(0, 1 << 32, 64) for _ in range(64)]         # sums wrap mod 2^32
    rows += [rng.integers(0, 4, 64) for _ in range(16)]
    rows = np.array(rows, dtype=np.uint32)
    want = (np.cumsum(rows.astype(np.uint64), axis=1) & 0xFFFFFFFF).astype(np.uint32)
    assert np.array_equal(units.wave_incl_scan(rows), want)


# ---- the value of the lane below ----------------------------------------------------------------------------------------------
def test_lane_up1(units):
    rng = np.random.default_rng(110)
    fills = [0, 1, 0xFFFFFFFF, 0x80000000, 0x12345678, 63]
    rows, fill = [], []
    for f in fills:
        rows += [np.arange(64), np.arange(64) + 0xFFFFFF00, rng.integers(0, 1 << 32, 64)]
        fill += [f] * 3
    rows, fill = np.array(rows, dtype=np.uint32), np.array(fill, dtype=np.uint32)
    want = np.concatenate([fill[:, None], rows[:, :63]], axis=1)
    assert np.array_equal(units.lane_up1(rows, fill), want)


# ---- every bit doubled --------------------------------------------------------------------------------------------------------
def test_bitrep32(units):
    rng = np.random.default_rng(152)
    x = np.array([0, 0xFFFFFFFF] + [1 << k for k in range(32)] + [0xFFFFFFFF ^ (1 << k) for k in range(32)] +
                 list(rng.integers(0, 1 << 32, 256)), dtype=np.uint32)
    want = np.zeros(len(x), dtype=np.uint64)
    for k in range(32):
        want |= ((x.astype(np.uint64) >> np.uint64(k)) & np.uint64(1)) * np.uint64(3 << (2 * k))
    assert np.array_equal(units.bitrep32(x), want)


# ---- four threshold bits ------------------------------------------------------------------------------------------------------
def above4_values():
    level = F32(0.3)
    v = [0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, level, np.nextafter(level, F32(0)),
         np.nextafter(level, F32(1)), np.inf, -np.inf, np.nan]
    return np.array(v, dtype=F32)


def test_above4(units):
    rng = np.random.default_rng(76)
    V = above4_values()
    thr, acc, x = [], [], []
    for t in V:
        for rep in range(3):
            xs = V[rng.integers(0, len(V), (64, 4))]
            for lane in range(len(V)):                       # every value in each of the four positions
                for j in range(4):
                    xs[lane + rep * len(V), j] = V[(lane + j * (rep + 1)) % len(V)]
            a = rng.integers(0, 1 << 32, 64)
            a[:4] = (0, 0xFFFFFFFF, 0xF0000000, 0x0FFFFFFF)
            thr.append(t)
            acc.append(a)
            x.append(xs)
    thr, acc, x = np.array(thr, dtype=F32), np.array(acc, dtype=np.uint32), np.array(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        bit = (x >= thr[:, None, None]).astype(np.uint32)    # IEEE float32, subnormals kept, a NaN on either side: 0
    want = ((acc.astype(np.uint64) << np.uint64(4)) & 0xFFFFFFFF).astype(np.uint32) | (bit[..., 0] << 3) | (bit[..., 1] << 2) | \
        (bit[..., 2] << 1) | bit[..., 3]
    assert bit.any() and not bit.all() and F32(2.0 ** -149) >= F32(-0.0)
    assert np.array_equal(units.above4(acc, x, thr), want)


# ---- |IQ|^2 of a complex64 sample ---------------------------------------------------------------------------------------------
def test_mag2(units):
    r, i = TC.complex64_pairs()
    want = TC.ref_mag2(r, i)
    assert np.any((want > 0) & (want < np.finfo(F32).tiny)) and np.any(np.isinf(want))
    TC.assert_bits(units.mag2(r, i), want, "adsb_mag2")
    nan_r = f32([QNAN, 0x3F800000, QNAN, SNAN, 0xFFC00000, 0x7F800000])
    nan_i = f32([0x3F800000, QNAN, QNAN, 0, 0x00000001, 0xFFC00001])
    assert np.all(np.isnan(units.mag2(nan_r, nan_i)))        # NaN inputs: a NaN, whichever


# ---- the 16-chip preamble test ------------------------------------------------------------------------------------------------
HALVES = (1, 2, 4, 10, -3, -10)      # the compile-time instances, and the run-time instance at 3 and 10 samples per chip
HIGH, LOW = (0, 2, 7, 9), (1, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15)


def chips_ref(taps):
    """chip k is tap[k] > f32(tap[0] / 2), a NaN compares false; the chips must spell 0x285"""
    taps = np.asarray(taps, dtype=F32)
    with np.errstate(invalid="ignore"):
        hp = taps[:, 0] * F32(0.5)
        chips = taps > hp[:, None]
    return (chips.astype(np.uint32) << np.arange(16, dtype=np.uint32)).sum(axis=1) == 0x285


def ideal(amp=1.0, low=0.0):
    t = np.full(16, low, dtype=F32)
    t[list(HIGH)] = amp
    return t


def chips_edge_rows():
    rows = []
    amp = F32(0.75)
    hp = amp * F32(0.5)
    for k in range(1, 16):                                   # a tap at tap[0]/2 exactly, one float32 step above, one below
        for v in (hp, np.nextafter(hp, F32(1)), np.nextafter(hp, F32(0))):
            t = ideal(amp)
            t[k] = v
            rows.append(t)
    for bits in (1, 3, 0x7F800000, 0, 0xBF800000, QNAN):     # tap[0] = 2^-149, 3 * 2^-149, +inf, 0, -1, NaN
        a = f32(bits)
        for low_bits in (0, 1, 2, 3, 0x80000000):
            t = ideal(a, f32(low_bits))
            rows.append(t)
            t = t.copy()
            t[list(HIGH[1:])] = F32(1.0)
            rows.append(t)
    for nan in (QNAN, SNAN, 0xFFC00000, 0xFFA00000):
        for k in range(1, 16):                               # a NaN in a chip that must be high / must be low
            t = ideal()
            t[k] = f32(nan)
            rows.append(t)
            if k in LOW:                                     # ... which must not hide another low chip that is high
                for other in LOW:
                    if other != k:
                        u = t.copy()
                        u[other] = F32(0.875)
                        rows.append(u)
        t = ideal()
        t[list(LOW)] = f32(nan)                              # all twelve low chips NaN
        rows.append(t)
        t = t.copy()
        t[0] = f32(nan)
        rows.append(t)
    return np.array(rows, dtype=F32)


def is_signalling(x):
    b = np.asarray(x, dtype=F32).view(np.uint32)
    return ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0) & ((b & 0x00400000) == 0)


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "computed"])
@pytest.mark.parametrize("half", HALVES)
def test_chips_match_every_pattern(units, half, raw):
    m = np.arange(1 << 16, dtype=np.uint32)
    taps = np.where((m[:, None] >> np.arange(16, dtype=np.uint32)) & 1, F32(1.0), F32(0.25)).astype(F32)
    want = chips_ref(taps)
    assert want.sum() == 1 and want[0x285]                   # only 0x285 matches
    got = units.chips_match(half, taps, raw)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "computed"])
@pytest.mark.parametrize("half", HALVES)
def test_chips_match_edges(units, half, raw):
    """raw: samples as the caller handed them over (|IQ|^2 floats), signalling NaNs among them.  computed: the instance of the
    formats that compute their samples -- arithmetic returns no signalling NaN, so those rows are not its input."""
    taps = chips_edge_rows()
    assert is_signalling(taps).any(axis=1).sum() > 100
    if not raw:
        taps = taps[~is_signalling(taps).any(axis=1)]
    want = chips_ref(taps)
    assert want.any() and not want.all()
    got = units.chips_match(half, taps, raw)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), [(int(b), bool(got[b]), taps[b].view(np.uint32).tolist()) for b in bad[:3]])


def test_a_signalling_nan_beside_a_high_low_chip_through_k_detect():
    """the finding of test_chips_match_edges at the level of a whole stream of |IQ|^2 floats: a burst whose preamble has a low
    chip high is no burst, also when the chip beside it is a signalling NaN; emulated k_detect against the C oracle"""
    from gr_adsb_amd import modulator
    from helpers import assert_recs_equal
    from oracle import c_oracle
    rng = np.random.default_rng(3)
    env = modulator.burst_waveform(modulator.make_frame(17, rng), 2)
    clean = np.full(900, 1e-4, dtype=F32)
    clean[300:300 + len(env)] += F32(0.5) * env.astype(F32)
    want = c_oracle.canonical(clean, 2, 0.01)
    assert len(want) == 1 and want["offset"][0] == 300      # tap k of its preamble is sample 300 + k
    seen = 0
    for nan_chip, high_chip in ((1, 3), (3, 1), (4, 3), (5, 6), (6, 5), (8, 10), (11, 12), (13, 14), (15, 14)):
        for nan in (SNAN, 0xFFA00000, QNAN):
            x = clean.copy()
            x[300 + high_chip] = F32(0.5)
            x[300 + nan_chip] = f32(nan)
            want = c_oracle.canonical(x, 2, 0.01)
            recs, _ = simlib.sim_canonical(1, x, 2e6, 0.01)
            assert_recs_equal(recs, want, "NaN %08x at chip %d, chip %d high" % (nan, nan_chip, high_chip))
            seen += len(want) == 0
    assert seen > 0, "the planted chip does spoil the preamble"
