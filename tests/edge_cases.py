"""One generator of edge cases for every k_detect instance, shared by the emulator (test_sim_edges.py) and the GPU
(test_gpu_edges.py) matrices: thresholds at and around the values the kernels special-case, stream shapes that reach
the plateau (k_longrun) and stream-end paths, lengths around every 16-byte load and tile, extreme integer values and
scales on both sides of the power-of-two instances' range.

cases(fmt, scale, sps) yields (name, data, x, thr): `data` in the wire format (FORMATS), `x` the oracle's float32 |IQ|^2
of the same bytes (the input of oracle.c_oracle.canonical), `thr` a float32 threshold."""
import numpy as np

from gr_adsb_amd import modulator as M
from oracle import adsb_oracle as O

# wire format -> (ADSB_FMT_* / emulator mode, default scale of the library: adsb_hip.hip, adsb_ctx::scale)
FORMATS = {"fc32": (0, None), "mag2": (1, None), "sc16": (2, 1.0 / 32768.0), "sc8": (3, 1.0 / 128.0), "cu8": (4, 1.0 / 255.0)}
LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 239, 240, 241, 1023, 1024, 1025, 4095, 4096, 4097, 4111, 4112)
SHORT_LENGTHS = (1, 7, 9, 17, 241, 4097)
# simlib.kernel_geometry() (test_sim_edges.py checks them against the compiled header): k_detect's tile and its forward halo --
# the body a wavefront converts in registers for the tile at t0 is samples [t0 + FWD, t0 + FWD + TILE), t0 a multiple of TILE
TILE, FWD = 1024, 256


def _f32(v):
    return float(np.float32(v))


def scales(fmt):
    """(label, scale) pairs for an integer format: the library default, the two ends of the power-of-two range of the
    dot-product instances (frexp exponent -49 .. 49: 2^-50 .. 2^48) and the first scales past them, int8 squares that round
    in the subnormal range (2^-75, 3 * 2^-75), overflow to +inf (int16 at 2^70) and the values nobody should pass but
    adsb_set_format_scale accepts (0, negative, +inf, NaN).  The float formats have no scale: [(None, None)]."""
    if FORMATS[fmt][1] is None:
        return [(None, None)]
    s = [("default", FORMATS[fmt][1]), ("2^-50", 2.0 ** -50), ("2^48", 2.0 ** 48), ("2^-51", 2.0 ** -51), ("2^49", 2.0 ** 49),
         ("2^-75", 2.0 ** -75), ("3*2^-75", 3.0 * 2.0 ** -75)]
    if fmt == "sc16":
        s.append(("2^70", 2.0 ** 70))
    s += [("0", 0.0), ("-1/128", -1.0 / 128.0), ("inf", float("inf")), ("nan", float("nan"))]
    return [(k, _f32(v)) for k, v in s]


def is_pow2(scale):
    """The library's scale_is_pow2 (adsb_hip.hip): the scales that run the int8 / uint8 dot-product instances."""
    m, e = np.frexp(np.float32(scale))
    return bool(m == 0.5 and -50 < e < 50)


def _bursts(rng, n, sps, amp, starts, last_bit0=False):
    """integer I, Q (int64) of n samples: noise of +-2 LSB, a Mode S burst of amplitude `amp` LSB at each start.
    last_bit0: every burst's 112th bit is 0, so its last sample is high (PPM: bit 0 = low chip, then high chip)."""
    i = rng.integers(-2, 3, n)
    q = rng.integers(-2, 3, n)
    for k, pos in enumerate(starts):
        if pos >= n:
            continue
        bits = M.make_frame(17 if k % 2 == 0 else 11, rng)
        if last_bit0:
            bits[-1] = 0
        env = M.burst_waveform(bits, sps)
        e = min(n, pos + len(env))
        on = env[:e - pos] > 0
        ph = rng.random() * 2 * np.pi
        a = amp[k % len(amp)]
        i[pos:e][on] += int(round(a * np.cos(ph)))
        q[pos:e][on] += int(round(a * np.sin(ph)))
    return i, q


def encode(fmt, i, q, scale):
    """Integer components -> (wire-format data, oracle |IQ|^2).  sc16 carries them times 256, the float formats times 2^-7."""
    iq = np.empty(2 * len(i), dtype=np.int64)
    iq[0::2], iq[1::2] = i, q
    if fmt == "sc8":
        d = np.clip(iq, -128, 127).astype(np.int8)
        return d, O.mag2_iq8(d, scale)
    if fmt == "cu8":
        d = np.clip(iq + 128, 0, 255).astype(np.uint8)
        return d, O.mag2_iq8(d, scale, offset_binary=True)
    if fmt == "sc16":
        d = np.clip(iq * 256, -32768, 32767).astype(np.int16)
        return d, O.mag2_iq16(d, scale)
    c = np.empty(len(i), dtype=np.complex64)
    c.real = np.float32(i) * np.float32(2.0 ** -7)
    c.imag = np.float32(q) * np.float32(2.0 ** -7)
    x = O.mag2(c)
    return (c if fmt == "fc32" else x), x


def unit2(fmt, scale):
    """|IQ|^2 of one LSB of the format at this scale: s^2 (sc16: (256 s)^2, floats: 2^-14), rounded once from float64."""
    if FORMATS[fmt][1] is None:
        return 2.0 ** -14
    u = (256.0 if fmt == "sc16" else 1.0) * float(np.float32(scale))
    if fmt == "cu8":
        u *= 2.0                        # one offset-binary step is 2 in 2 u8 - 255
    with np.errstate(all="ignore"):
        return u * u


def _thr(v):
    with np.errstate(all="ignore"):
        return np.float32(v)


def threshold_cases(x, u2, levels):
    """The thresholds k_detect special-cases: 0.0, -0.0 (thr > 0 decides between the quiet-body skip and the exact path),
    a negative one, NaN, +inf, the smallest subnormal, an |IQ|^2 level present in the stream and its float32 neighbours."""
    t = [("thr 0.0", _thr(0.0)), ("thr -0.0", _thr(-0.0)), ("thr -1", _thr(-1.0)), ("thr nan", _thr(np.nan)),
         ("thr +inf", _thr(np.inf)), ("thr 2^-149", _thr(2.0 ** -149)), ("thr 400 lsb^2", _thr(400.0 * u2))]
    if levels:
        lv = np.float32(levels[0])
        t += [("thr = level", lv), ("thr below level", np.nextafter(lv, np.float32(-np.inf))),
              ("thr above level", np.nextafter(lv, np.float32(np.inf)))]
    return t


def cases(fmt, scale, sps, full=True):
    """Edge cases of one format at one scale and rate.  full=False: the thresholds, the shapes and SHORT_LENGTHS only
    (what the non-default scales run)."""
    rng = np.random.default_rng(sps * 1000 + (int(np.float32(scale).view(np.uint32)) if scale is not None else 7) % 1000 +
                                sum(map(ord, fmt)))
    L = 120 * sps                                   # one burst: 8 preamble + 112 data symbols
    u2 = unit2(fmt, scale)
    amp = (40, 60, 90)
    base_n = 6 * L + 2500
    i, q = _bursts(rng, base_n, sps, amp, [300, 300 + L + 100 * sps, 300 + 3 * L, base_n - L - 50])
    d, x = encode(fmt, i, q, scale)
    levels = [float(x[300])] if np.isfinite(x[300]) else []         # the first burst's first preamble sample
    thr0 = _thr(400.0 * u2)                                         # 20 LSB: between the noise and every burst

    for name, t in threshold_cases(x, u2, levels):
        yield name, d, x, t

    # shapes
    qi, qq = rng.integers(-2, 3, 3000), rng.integers(-2, 3, 3000)
    yield ("all quiet",) + encode(fmt, qi, qq, scale) + (thr0,)
    n = 3 * TILE + 2 * L + 4000                                     # a carrier longer than the LDS window, over several tiles
    ci, cq = _bursts(rng, n, sps, amp, [200, n - L - 100])
    ci[L + 400:L + 400 + 3 * TILE + 700] += 70
    yield ("carrier over tiles",) + encode(fmt, ci, cq, scale) + (thr0,)
    ci, cq = _bursts(rng, 4000, sps, amp, [600])
    ci[:50] += 80
    ci[-40:] += 80
    yield ("starts and ends high",) + encode(fmt, ci, cq, scale) + (thr0,)
    ci, cq = _bursts(rng, 2 * L + 600, sps, amp, [0, L + 200])
    yield ("burst at 0",) + encode(fmt, ci, cq, scale) + (thr0,)

    # extreme integer values as the bursts' high chips
    if fmt in ("sc16", "sc8", "cu8"):
        vi, vq = _bursts(rng, 3 * L + 1500, sps, (30,), [100, 100 + L + 300, 100 + 2 * L + 600])
        hi = np.flatnonzero(np.abs(vi) + np.abs(vq) > 15)
        vi[hi] = -128                                     # int8 -128, uint8 0, int16 -32768 (after the sc16 * 256)
        vq[hi] = -128
        if fmt == "cu8":
            vi[hi[1::3]] = 127                            # uint8 255 mixed in
        yield ("extreme values",) + encode(fmt, vi, vq, scale) + (thr0,)

    # lengths: a burst at sample 0 and one whose last sample (high) is the stream's last, so that every sample up to n - 1
    # reaches the records (the last bit of that burst); the 8-bit loads hold 8 samples, int16 4, complex64 2, floats 4
    for n in (LENGTHS if full else SHORT_LENGTHS):
        starts = [0] if n < L else ([n - L] if n < 2 * L + 64 else [0, n - L])
        li, lq = _bursts(rng, n, sps, amp, starts, last_bit0=True)
        dd, xx = encode(fmt, li, lq, scale)
        yield "n=%d" % n, dd, xx, thr0
        if full and n in (1, 7, 9, 17, 241, 1025, 4097):
            yield "n=%d thr -1" % n, dd, xx, _thr(-1.0)

    if fmt in ("fc32", "mag2"):
        yield from _float_cases(fmt, rng, sps)


def _float_cases(fmt, rng, sps):
    """complex64 / |IQ|^2: subnormal components, subnormal and normal |IQ|^2 in one stream, near-overflow components;
    for |IQ|^2 input: -0.0 preamble pulses on a negative floor at thr 0.0 (see negzero_pulses)."""
    L = 120 * sps
    n = 6 * L + 3000
    i, q = _bursts(rng, n, sps, (40, 60, 90), [200, 200 + 2 * L, 200 + 4 * L])
    for label, k, thr in (("subnormal", -72, 2.0 ** -144 * 400), ("near overflow", 56, 2.0 ** 112 * 400)):
        c = np.empty(n, dtype=np.complex64)
        with np.errstate(all="ignore"):
            c.real = np.float32(i) * np.float32(2.0 ** k)
            c.imag = np.float32(q) * np.float32(2.0 ** k)
            x = O.mag2(c)
        yield label, (c if fmt == "fc32" else x), x, _thr(thr)
    # mixed: the second half of the stream 2^60 times weaker (components ~2^-67: |IQ|^2 subnormal)
    c = np.empty(n, dtype=np.complex64)
    f = np.where(np.arange(n) < 200 + 3 * L, np.float32(2.0 ** -7), np.float32(2.0 ** -67))
    c.real = np.float32(i) * f
    c.imag = np.float32(q) * f
    x = O.mag2(c)
    assert np.any((x > 0) & (x < np.finfo(np.float32).tiny)) and np.any(x > 1e-3)
    yield "subnormal and normal mixed", (c if fmt == "fc32" else x), x, _thr(2.0 ** -134 * 400)
    yield "subnormal and normal mixed, thr 2^-149", (c if fmt == "fc32" else x), x, _thr(2.0 ** -149)
    if fmt == "mag2":
        x = negzero_pulses(sps)
        yield "-0.0 pulses, thr 0.0", x, x, _thr(0.0)


def negzero_pulses(sps, ntiles=64):
    """|IQ|^2 floats over `ntiles` tiles: a negative floor with preambles whose pulse at chip 0 starts with a -0.0 sample
    (>= 0.0: at thr 0.0 the pulse rises there, and its centre -- (rise + fall) // 2, framer.py:113 -- is the preamble's
    chip 0; rising one sample later it would be the next sample, which does not match).

    Chunks are whole tiles from sample 0, so the body a wavefront converts for tile t is [t TILE + FWD, (t + 1) TILE + FWD)
    whatever the chunk plan.  Every -0.0 sample is the last sample of the body of an even tile t, and its pulse's positive
    samples lie in the next body: body t holds no sample whose bit pattern is >= 0, so only the exact path (thr_pos false)
    sees the rise.  The -0.0 sample belongs to tile t + 1, which takes its mask from body t only when t + 1 is not the first
    tile of a unit (a unit's first tile computes its head exactly): callers must run this with chunks of two tiles or more
    (test_sim_edges / test_gpu_edges check the plan)."""
    h = sps // 2
    m = 2 if h == 1 else 1                  # the pulse: -0.0, then 2m positive samples (chip 1 of h = 1 inside it, low)
    n = ntiles * TILE
    rng = np.random.default_rng(sps)
    x = -(np.float32(0.25) + rng.random(n, dtype=np.float32))
    r = np.arange(2, ntiles - 3, 2) * TILE + TILE + FWD - 1           # the -0.0 samples
    c = r + m                                                         # the preambles' chip 0
    x[r] = np.float32(-0.0)
    for k in range(1, 2 * m + 1):
        x[r + k] = np.float32(1.0)
    if h == 1:
        x[c + 1] = np.float32(0.125)    # chip 1: in the pulse (>= 0), not above half the centre
    for k in (2, 7, 9):
        for j in range(h):
            x[c + k * h + j] = np.float32(1.0)
    return x
