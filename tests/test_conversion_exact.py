"""The integer and complex input conversions pinned to an independent reference.

oracle.adsb_oracle defines |IQ|^2 of every wire format in NumPy float32 (mag2, mag2_iq16, mag2_iq8), and the C oracle, the
emulator and the GPU are all compared against it.  Here each of those is recomputed in float64 with a cast to float32 after
every single operation: the operands are float32, and since 53 >= 2 * 24 + 2 every product and sum rounded that way is the
correctly rounded float32 result, subnormals included.  The emulated k_detect conversion (simlib.convert8, body_convert of
modes 3-6) is checked against the same reference."""
import numpy as np
import pytest

import edge_cases as E
import simlib
from oracle import adsb_oracle as O

F32 = np.float32
SCALES = sorted({s for f in ("sc16", "sc8", "cu8") for _, s in E.scales(f)} |
                {float(F32(v)) for v in (1.0 / 127.0, 1.0 / 255.0, 2.0 ** -8, 2.0 ** -149, 2.0 ** -126, 3.4e38, -2.0 ** -7)},
                key=lambda v: (np.isnan(v), v))


def _r(v):
    """float64 -> float32, one rounding"""
    with np.errstate(all="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float32)


def _mul(a, b):
    with np.errstate(all="ignore"):
        return _r(np.asarray(a, np.float64) * np.asarray(b, np.float64))


def _add(a, b):
    with np.errstate(all="ignore"):
        return _r(np.asarray(a, np.float64) + np.asarray(b, np.float64))


def ref_mag2(re, im):
    return _add(_mul(re, re), _mul(im, im))


def ref_components(ints, scale):
    """exact integers -> float32 component: one rounded multiply by float32(scale)"""
    return _mul(_r(np.asarray(ints, np.float64)), F32(scale))


def ref_iq8(b, scale, offset_binary):
    c = 2 * np.asarray(b, np.int64) - 255 if offset_binary else np.asarray(b, np.int64)
    v = ref_components(c, scale)
    return ref_mag2(v[0::2], v[1::2])


def ref_iq16(q, scale):
    v = ref_components(np.asarray(q, np.int64), scale)
    return ref_mag2(v[0::2], v[1::2])


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%s: %d differ, first at %d: %r vs %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def every_pair(dtype):
    k = np.arange(65536, dtype=np.uint32)
    return np.stack([k & 0xFF, k >> 8], axis=1).astype(np.uint8).reshape(-1).view(dtype)


def test_reference_is_not_flushed():
    """the reference itself: float64 -> float32 keeps subnormals (a flushing FPU mode would make it vacuous)"""
    assert _r(2.0 ** -149).view(np.uint32) == 1
    assert _mul(F32(2.0 ** -75), F32(2.0 ** -74)).view(np.uint32) == 1
    assert _mul(F32(2.0 ** -75), F32(2.0 ** -75)).view(np.uint32) == 0            # 2^-150: a tie, to even


@pytest.mark.parametrize("scale", SCALES)
def test_int8_every_pair(scale):
    b = every_pair(np.int8)
    assert_bits(O.mag2_iq8(b, scale), ref_iq8(b, scale, False), "int8, scale %r" % scale)


@pytest.mark.parametrize("scale", SCALES)
def test_uint8_every_pair(scale):
    b = every_pair(np.uint8)
    assert_bits(O.mag2_iq8(b, scale, offset_binary=True), ref_iq8(b, scale, True), "uint8, scale %r" % scale)


def int16_edge_set():
    e = [-32768, -32767, -1, 0, 1, 32767]
    for k in range(16):
        e += [2 ** k - 1, 2 ** k + 1, -(2 ** k) - 1, -(2 ** k) + 1]
    e = np.array(sorted({v for v in e if -32768 <= v <= 32767}), dtype=np.int64)
    a, b = np.meshgrid(e, e)
    rng = np.random.default_rng(16)
    edge = np.stack([a.ravel(), b.ravel()], axis=1).reshape(-1)
    return np.concatenate([edge, rng.integers(-32768, 32768, 2 * (1 << 20))]).astype(np.int16)


@pytest.mark.parametrize("scale", SCALES)
def test_int16_edges_and_random(scale):
    q = int16_edge_set()
    assert_bits(O.mag2_iq16(q, scale), ref_iq16(q, scale), "int16, scale %r" % scale)


def complex64_pairs():
    """(re, im) float32: every sign and pairing of magnitudes from the smallest subnormal to the largest finite value, and
    65536 random pairs over the whole exponent range"""
    rng = np.random.default_rng(64)
    mags = [0.0, 2.0 ** -149, 2.0 ** -140, 2.0 ** -126, 2.0 ** -75, 2.0 ** -63, 2.0 ** -62, 1.0, 2.0 ** 63, 1.8446743e19,
            2.0 ** 64, 3.4028235e38]
    v = np.array([s * m for m in mags for s in (1.0, -1.0)], dtype=np.float32)
    a, b = np.meshgrid(v, v)
    r = np.concatenate([a.ravel(), np.ldexp(rng.random(1 << 16), rng.integers(-150, 128, 1 << 16)).astype(np.float32)])
    i = np.concatenate([b.ravel(), np.ldexp(rng.random(1 << 16), rng.integers(-150, 128, 1 << 16)).astype(np.float32)])
    return r, i


def test_complex64_subnormal_and_near_overflow():
    r, i = complex64_pairs()
    iq = np.empty(len(r), np.complex64)
    iq.real, iq.imag = r, i
    with np.errstate(all="ignore"):
        got = O.mag2(iq)
    want = ref_mag2(r, i)
    assert np.any((want > 0) & (want < np.finfo(np.float32).tiny)) and np.any(np.isinf(want))
    assert_bits(got, want, "complex64")


@pytest.mark.parametrize("scale", SCALES)
def test_emulated_body_convert_8bit(scale):
    """k_detect's in-register conversion of 16-byte loads (modes 3, 4; 5 and 6 -- the dot-product instances -- wherever the
    library would choose them, i.e. at power-of-two scales inside its range)"""
    for mode, dtype, ob in ((3, np.int8, False), (4, np.uint8, True)):
        b = every_pair(dtype)
        want = ref_iq8(b, scale, ob)
        assert_bits(simlib.convert8(mode, b, scale), want, "body_convert<%d>, scale %r" % (mode, scale))
        if E.is_pow2(scale):
            assert_bits(simlib.convert8(mode + 2, b, scale), want, "body_convert<%d>, scale %r" % (mode + 2, scale))
