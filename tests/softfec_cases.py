"""Hand-built records over a hand-built float buffer for the soft-decision CRC repair (include/adsb_hip.h: SOFT REPAIR): every
record sits at a seam of the rule.  Shared by tests/test_softfec.py (the emulated kernels and the host rule) and the GPU tests.
Each burst occupies one slot of the buffer: the sample of the set half of bit i is 1.0, the other one is the bit's key, so that
key = lo / hi is that float exactly."""
import json
import os

import numpy as np

import softfec_replay as SR

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHT6 = os.path.join(HERE, "golden", "softfec_weight6.json")
N_SAMPLES = 1 << 12


def frame(df, rng, fixed=None):
    """a parity-consistent DF 11/17/18/19 reply, as 112 bits (a short reply: random bits behind bit 55); fixed: {bit: value}"""
    L = SR.length_of(df)
    bits = rng.integers(0, 2, 112).astype(np.uint8)
    bits[:5] = [(df >> (4 - i)) & 1 for i in range(5)]
    for i, v in (fixed or {}).items():
        bits[i] = v
    bits[L - 24:L] = 0
    S = SR.syndrome(bits, L)
    bits[L - 24:L] = [(S >> (23 - i)) & 1 for i in range(24)]
    assert SR.syndrome(bits, L) == 0
    return bits


def find_weight6(lo_bit=5, L=112):
    """The first codeword of weight 6 of the Mode S CRC whose positions are all >= lo_bit, by a meet-in-the-middle search over
    triples of x^j mod G: two disjoint triples with the same XOR.  -> six ascending bit positions (first triple, second triple)."""
    js = range(0, L - lo_bit)
    seen = {}
    for a in js:
        for b in range(a + 1, L - lo_bit):
            ab = SR.R[a] ^ SR.R[b]
            for c in range(b + 1, L - lo_bit):
                v = ab ^ SR.R[c]
                other = seen.get(v)
                if other is not None and not set(other) & {a, b, c}:
                    one = sorted(L - 1 - j for j in other)
                    two = sorted(L - 1 - j for j in (a, b, c))
                    return one, two
                seen.setdefault(v, (a, b, c))
    return None


def weight6():
    d = json.load(open(WEIGHT6))
    return d["first"], d["second"]


class Buffer:
    """a float32 |IQ|^2 buffer of N_SAMPLES samples cut into burst slots of 120 * sps samples"""

    def __init__(self, sps, seed=5):
        self.sps, self.rng = sps, np.random.default_rng(seed)
        self.x = (self.rng.random(N_SAMPLES, dtype=np.float32) * np.float32(0.01)).astype(np.float32)
        self.next = 3
        self.recs, self.names = [], []

    def slot(self):
        p = self.next
        self.next += 120 * self.sps
        assert p + 119 * self.sps + self.sps // 2 < N_SAMPLES, "buffer full"
        return p

    def burst(self, p, bits, key):
        """samples of the burst at p: bit i reads bits[i] and has weakness key[i]"""
        for i in range(112):
            s1 = p + 8 * self.sps + i * self.sps
            s0 = s1 + self.sps // 2
            hi, lo = np.float32(1.0), np.float32(key[i])
            self.x[s1], self.x[s0] = (hi, lo) if bits[i] else (lo, hi)

    def sample(self, p, i, x1, x0):
        s1 = p + 8 * self.sps + i * self.sps
        self.x[s1], self.x[s1 + self.sps // 2] = x1, x0

    def record(self, name, p, bits, flags=None):
        """a delivered record at p with these bits; flags: DEMOD | the pre-filter bits unless given"""
        r = np.zeros((), dtype=SR.REC_DTYPE)
        r["offset"], r["peak"], r["median"] = p + 1000, 1.0, 0.01          # origin 1000
        r["bits"] = SR.pack(bits)
        r["flags"] = (SR.DEMOD | 2 | SR.prefilter_flags(bits)) if flags is None else flags
        self.recs.append(r)
        self.names.append(name)

    def records(self):
        return np.array(self.recs, dtype=SR.REC_DTYPE)


ORIGIN = 1000


def strong_keys(rng):
    """keys of confident bits: all below 0.2, pairwise distinct"""
    return (rng.permutation(112).astype(np.float32) * np.float32(0.001) + np.float32(0.01)).astype(np.float32)


def flipped(bits, idx):
    b = bits.copy()
    b[list(idx)] ^= 1
    return b


def build(sps=2):
    """-> Buffer with the named records of every seam (sps 2), or the three that fit (sps 10)"""
    B = Buffer(sps)
    rng = B.rng

    def weak(key, idx, start=0.9, step=-0.01):
        for k, i in enumerate(idx):
            key[i] = np.float32(start + step * k)

    # one wrong bit that is the weakest
    f = frame(17, rng); key = strong_keys(rng); weak(key, [40, 7, 99, 20, 64, 63, 88, 5, 77])   # ranks 0..8
    p = B.slot(); B.burst(p, flipped(f, [40]), key); B.record("one_weakest", p, flipped(f, [40]))
    B.truth = {"one_weakest": f}
    # three scattered wrong bits inside the 8 weakest
    f3 = frame(17, rng); key = strong_keys(rng); weak(key, [30, 91, 12, 70, 8, 101, 55, 66])
    p = B.slot(); B.burst(p, flipped(f3, [91, 8, 66]), key); B.record("three_scattered", p, flipped(f3, [91, 8, 66]))
    B.truth["three_scattered"] = f3
    # a clean reply, and what never qualifies, on one slot
    fc = frame(18, rng); key = strong_keys(rng); weak(key, [10, 20, 30])
    p = B.slot(); B.burst(p, fc, key)
    B.record("clean", p, fc)
    bad = flipped(fc, [10])
    B.record("no_demod", p, bad, flags=(2 | SR.prefilter_flags(bad)))
    B.record("fec_df", p, bad, flags=(SR.DEMOD | 2 | SR.prefilter_flags(bad) | SR.FEC_DF))
    ap = bad.copy(); ap[:5] = [1, 0, 1, 0, 0]                                                   # DF 20
    B.record("df20", p, ap)
    if sps != 2:
        return B
    # one wrong bit at rank n_weak: just outside
    f = frame(17, rng); key = strong_keys(rng); weak(key, [40, 7, 99, 20, 64, 63, 88, 5, 77])
    p = B.slot(); B.burst(p, flipped(f, [77]), key); B.record("one_outside", p, flipped(f, [77]))
    # a key tie across the n_weak boundary: ranks 7 and 8 hold the same key; the lower bit index is kept
    for name, wrong in (("tie_lower_wrong", 33), ("tie_higher_wrong", 34)):
        f = frame(17, rng); key = strong_keys(rng); weak(key, [50, 51, 52, 53, 54, 56, 57])
        key[33] = key[34] = np.float32(0.5)
        p = B.slot(); B.burst(p, flipped(f, [wrong]), key); B.record(name, p, flipped(f, [wrong]))
    # lane and word seams: bits 5, 63, 64, 111
    f = frame(19, rng); key = strong_keys(rng); weak(key, [111, 5, 64, 63, 17, 18])
    p = B.slot(); B.burst(p, flipped(f, [5, 63, 64, 111]), key); B.record("seams", p, flipped(f, [5, 63, 64, 111]))
    B.truth["seams"] = f
    # a wrong bit 3 on a DF 17: reads as DF 19; bits 0-4 are never candidates
    f = frame(17, rng); key = strong_keys(rng); weak(key, [3, 9, 10])
    p = B.slot(); B.burst(p, flipped(f, [3]), key); B.record("df_bit", p, flipped(f, [3]))
    # DF 11: the weakest bits lie at 56 and beyond, the wrong bit is 55
    f = frame(11, rng); key = strong_keys(rng); weak(key, [60, 70, 80, 90, 100, 110, 56, 57, 58], start=0.99, step=-0.001)
    weak(key, [55, 6], start=0.6)
    p = B.slot(); B.burst(p, flipped(f, [55]), key); B.record("df11", p, flipped(f, [55]))
    B.truth["df11"] = f
    # a codeword of weight 6: two 3-subsets match; the smaller mask wins, in both rank orders
    one, two = weight6()
    for name, order in (("weight6_true_first", one + two), ("weight6_other_first", two + one)):
        f = frame(17, rng); key = strong_keys(rng); weak(key, order)
        p = B.slot(); B.burst(p, flipped(f, one), key); B.record(name, p, flipped(f, one))
        B.truth[name] = f
    # samples that have no quotient: 0/0, NaN, +inf, negative floats.  The true reply agrees with what those samples read,
    # except at 21 and 26 -- the two bits of key 1
    f = frame(17, rng, fixed={21: 1, 22: 0, 23: 0, 24: 1, 25: 0, 26: 0}); key = strong_keys(rng)
    bits = flipped(f, [21, 26])
    p = B.slot(); B.burst(p, bits, key)
    B.sample(p, 21, 0.0, 0.0)                               # key 1, reads 0
    B.sample(p, 22, np.nan, 0.5)                            # key 0, reads 0
    B.sample(p, 23, np.nan, np.nan)                         # key 1, reads 0
    B.sample(p, 24, np.inf, 1.0)                            # key 0, reads 1
    B.sample(p, 25, -0.5, 0.25)                             # key 0, reads 0
    B.sample(p, 26, -1.0, -2.0)                             # key 1, reads 1
    B.record("no_quotient", p, bits)
    B.truth["no_quotient"] = f
    # five wrong bits at ranks 11..15 of sixteen
    f = frame(17, rng); key = strong_keys(rng)
    order = [31, 45, 6, 86, 97, 14, 69, 104, 23, 58, 75, 110, 36, 65, 62, 11]
    weak(key, order)
    p = B.slot(); B.burst(p, flipped(f, order[11:]), key); B.record("five_deep", p, flipped(f, order[11:]))
    B.truth["five_deep"] = f
    return B


RULES = {
    "default": dict(n_weak=8, max_flips=3, min_key=0.0),
    "two_flips": dict(n_weak=8, max_flips=2, min_key=0.0),
    "caps": dict(n_weak=16, max_flips=5, min_key=0.0),
    "one_weak": dict(n_weak=1, max_flips=3, min_key=0.0),
    "min_key_between": dict(n_weak=8, max_flips=3, min_key=0.845),
    "min_key_one": dict(n_weak=8, max_flips=3, min_key=1.0),
}


def slices_of(recs):
    """the records as adsb_demod_work's slices: (bits14, ok, local tag positions)"""
    fl = recs["flags"].astype(np.uint32)
    ok = ((fl & 0xE1) | ((fl & (SR.FEC_FIXED | SR.FEC_DF)) >> 13)).astype(np.uint8)
    return recs["bits"].copy(), ok, (recs["offset"] - ORIGIN).astype(np.int64)
