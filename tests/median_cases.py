"""noise_median (gr_adsb_amd/csrc/adsb_device.h) on chosen inputs: a plain reference, the case generators, and a plain statement
of which turn (adsb::MedianPath) a window must take.  Shared by tests/test_median.py (the SIMT emulator) and
tests/test_gpu_units.py (the MI355X): fixed seeds, the same arrays for every consumer.

A CHAIN is 1-8 windows handled by one wavefront in order: the hint starts at the chain's hint0 and is carried from window to
window (each window's lower-middle key is the next window's hint, 0 after an empty window).  A window is 128 float32 of which
the first nwin are valid; positions at or beyond nwin hold 0.0, as burst_from_window forms them."""
import numpy as np

F32 = np.float32
U32 = np.uint32
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 98, 99, 100)
WIN = 128
PATHS = ("hint_none", "hint_exact", "hint_below", "hint_above", "hint_refused",
         "one_16", "one_12", "one_8", "crowd_16", "crowd_12", "crowd_8", "bit_0",
         "upper_odd", "upper_exact_again", "upper_count", "upper_next")      # adsb::MedianPath, in order
HINTS, EXITS, UPPERS = PATHS[0:5], PATHS[5:12], PATHS[12:16]
NAN_EMPTY, NAN_WINDOW = 0xFFC00000, 0x7FC00000
K_ONE = 0xBF800000                # the key of 1.0: its low 16 bits are clear


def f32(bits):
    return np.asarray(bits, dtype=np.uint64).astype(U32).view(F32)


def bits_of(x):
    return np.asarray(x, dtype=F32).view(U32)


def key_of(x):
    """the order-preserving key of float32 values: the sign bit flipped for positive patterns, every bit for negative ones"""
    u = bits_of(x).astype(np.uint64)
    return np.where(u >> 31, u ^ 0xFFFFFFFF, u ^ 0x80000000).astype(np.uint64)


def unkey(k):
    k = np.asarray(k, dtype=np.uint64) & 0xFFFFFFFF
    return f32(np.where(k >> 31, k ^ 0x80000000, k ^ 0xFFFFFFFF))


def median_ref(window):
    """(bits of np.median as the device must give it, key of the lower middle).  Knows nothing of hints or paths."""
    w = np.asarray(window, dtype=F32)
    n = len(w)
    if n == 0:
        return NAN_EMPTY, 0
    s = w[np.argsort(key_of(w), kind="stable")]
    a = s[(n - 1) >> 1]
    if np.isnan(w).any():
        return NAN_WINDOW, int(key_of(a))
    with np.errstate(all="ignore"):
        if n & 1:
            m = F32(a + F32(0.0))
        else:
            m = F32(F32(F32(a + s[n >> 1]) * F32(0.5)) + F32(0.0))
    return int(bits_of(m)), int(key_of(a))


def predict(window, hint, quant):
    """The turns noise_median<quant> must take on this window with this hint, as a set of PATHS names, from the function's
    contract (adsb_device.h): the hint is tried iff it lies in [0x00800000, 0xFF000000) and is proved exact (quant) / within 2^23
    keys; the select then works on intervals of 2^16, 2^12, 2^8 keys counted from its base (0, the hint, or the hint - 2^23) and
    leaves at the first that holds one key, or four or more that are all equal; the upper middle of an even window."""
    w = np.asarray(window, dtype=F32)
    n = len(w)
    keys = np.full(WIN, 0xFFFFFFFF, dtype=np.uint64)         # lanes outside the window sort last
    keys[:n] = key_of(w)
    kt = (n - 1) >> 1
    K = int(np.sort(keys)[kt]) if n else 0
    out = set()
    base, exact = 0, False
    if not (0x00800000 <= hint < 0xFF000000):
        out.add("hint_none")
    elif quant and n and hint == K:
        out.add("hint_exact")
        exact = True
    elif n and hint <= K < hint + (1 << 23):
        out.add("hint_above")
        base = hint
    elif n and hint - (1 << 23) <= K < hint:
        out.add("hint_below")
        base = hint - (1 << 23)
    else:
        out.add("hint_refused")
    single = False
    if not exact:
        for sp, tag in ((1 << 16, "16"), (1 << 12, "12"), (1 << 8, "8")):
            lo = base + ((K - base) // sp) * sp
            inside = keys[(keys >= lo) & (keys < lo + sp)]
            if len(inside) == 1:
                out.add("one_" + tag)
                single = True
                break
            if len(inside) >= 4 and inside.min() == inside.max():
                out.add("crowd_" + tag)
                break
        else:
            out.add("bit_0")
    if n and not np.isnan(w).any():
        if n & 1:
            out.add("upper_odd")
        elif not single and int((keys <= K).sum()) >= kt + 2:
            out.add("upper_exact_again" if exact else "upper_count")
        else:
            out.add("upper_next")
    return out


class Chain:
    """name; windows: [float32[nwin]]; hint0; expect: None, or per window a set of PATHS names the case was built for -- a set,
    or {quant: set} where the two instances differ"""
    def __init__(self, name, windows, hint0=0, expect=None):
        self.name, self.hint0, self.expect = name, int(hint0) & 0xFFFFFFFF, expect
        self.windows = [np.ascontiguousarray(w, dtype=F32) for w in windows]
        assert 1 <= len(self.windows) <= 8 and all(len(w) <= 100 for w in self.windows), name
        assert expect is None or len(expect) == len(self.windows), name

    def expected(self, k, quant):
        e = self.expect[k] if self.expect else None
        return (e.get(quant, set()) if isinstance(e, dict) else e) or set()


# ---- value distributions: (rng, n) -> float32[n] ------------------------------------------------------------------------------
def _distinct(rng, n):
    return (rng.permutation(4096)[:n] + 1).astype(F32) * F32(2.0 ** -20) * F32(rng.uniform(1.0, 2.0))


def _equal(rng, n):
    return np.full(n, 0.25, dtype=F32)


def _levels(count):
    def gen(rng, n):
        return (rng.integers(0, count, n) + 1).astype(F32) * F32(2.0 ** -12)
    return gen


def _iq8(scale, offset_binary):
    def gen(rng, n):
        s = F32(scale)
        if offset_binary:
            c = (2 * rng.integers(125, 131, (2, n)) - 255).astype(F32)
        else:
            c = rng.integers(-3, 4, (2, n)).astype(F32)
        re, im = c[0] * s, c[1] * s
        return re * re + im * im                             # float32 throughout: mag2_iq8's arithmetic
    return gen


def _carrier(rng, n):
    return unkey(K_ONE + rng.integers(0, 256, n))           # 1.0 + j * 2^-23


def _negative(rng, n):
    return -_distinct(rng, n)


def _straddle(rng, n):
    v = np.concatenate([-_distinct(rng, n)[:n // 2], _distinct(rng, n)[:n - n // 2]])
    return rng.permutation(v).astype(F32)


def _zeros_mixed(rng, n):
    return rng.permutation(np.where(np.arange(n) < (n + 1) // 2, F32(-0.0), F32(0.0)).astype(F32))


def _zeros_negative(rng, n):
    return np.full(n, -0.0, dtype=F32)


def _subnormal(rng, n):
    return f32(rng.integers(1, 0x00800000, n))


def _with(at, bits):
    """distinct floats with one sample replaced by the pattern `bits` (a NaN) where the window reaches sample `at`"""
    def gen(rng, n):
        v = _distinct(rng, n)
        if at < n:
            v[at] = f32(bits)
        return v
    return gen


DISTRIBUTIONS = [
    ("distinct", _distinct), ("equal", _equal),
    ("levels2", _levels(2)), ("levels3", _levels(3)), ("levels4", _levels(4)), ("levels8", _levels(8)), ("levels256", _levels(256)),
    ("int8_128", _iq8(1.0 / 128, False)), ("int8_127", _iq8(1.0 / 127, False)),
    ("uint8_128", _iq8(1.0 / 128, True)), ("uint8_127", _iq8(1.0 / 127, True)),
    ("carrier", _carrier), ("negative", _negative), ("straddle", _straddle),
    ("zeros_mixed", _zeros_mixed), ("zeros_negative", _zeros_negative), ("subnormal", _subnormal),
    ("nan_at_0", _with(0, 0x7FC00000)), ("nan_at_64", _with(64, 0x7FC00000)), ("nan_at_99", _with(99, 0x7FC00000)),
    ("negative_nan", _with(1, 0xFFC00000)), ("signalling_nan", _with(2, 0x7FA00000)), ("negative_signalling_nan", _with(0, 0xFFA00000)),
]


def around(n, mid_keys, rng, d_lo=1 << 20, d_hi=1 << 20, pos=0):
    """float32[n], shuffled, whose keys are: mid_keys (ascending) with mid_keys[pos] at rank (n-1)>>1; below them one key d_lo
    under the first and distinct keys at least 2^20 further down; above them one key d_hi over the last and distinct keys at
    least 2^20 further up.  None if the middles do not fit."""
    kt = (n - 1) >> 1
    below, above = kt - pos, n - (kt - pos) - len(mid_keys)
    if below < 0 or above < 0:
        return None
    lo, hi = int(mid_keys[0]), int(mid_keys[-1])
    ks = [lo - d_lo - (j << 20) - (int(rng.integers(0, 1 << 19)) if j else 0) for j in range(below)]
    ks += list(mid_keys)
    ks += [hi + d_hi + (j << 20) + (int(rng.integers(0, 1 << 19)) if j else 0) for j in range(above)]
    assert min(ks) > 0x00800000 and max(ks) < 0xFF000000
    return unkey(rng.permutation(np.array(ks, dtype=np.uint64)))


def special_middles(rng):
    """windows whose middle one or two samples are given patterns, the rest filled below / above: (name, window)"""
    out = []

    def put(name, n, a, b, lo_fill, hi_fill):
        kt = (n - 1) >> 1
        w = np.empty(n, dtype=np.uint32)
        w[:kt], w[kt] = lo_fill, a
        w[kt + 1:] = hi_fill
        if n % 2 == 0:
            w[kt + 1] = b
        out.append(("%s_n%d" % (name, n), f32(rng.permutation(w))))

    neg1, big, inf, ninf = 0xBF800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000
    for n in (1, 2, 3, 4, 64, 65, 98, 99, 100):
        put("subnormal_1_3", n, 1, 3, 0, 0x00800000)
        put("subnormal_1_2", n, 1, 2, 0, 0x00800000)
        put("subnormal_3_4", n, 3, 4, 0x80000001, 0x00000007)
        put("negative_subnormal_3_1", n, 0x80000003, 0x80000001, neg1, 0)
        put("near_overflow", n, big, big, 0x3F800000, inf)
        put("near_overflow_half", n, 0x7F000000, 0x7F000000, 0x3F800000, big)
        put("negative_overflow", n, 0xFF7FFFFF, 0xFF7FFFFF, ninf, 0)
        put("inf_inf", n, inf, inf, 0x3F800000, inf)
        put("ninf_inf", n, ninf, inf, ninf, inf)
        put("ninf_finite", n, ninf, 0x3F800000, ninf, inf)
        put("negzero_poszero", n, 0x80000000, 0, neg1, 0x3F800000)
        put("negative_a_positive_b", n, 0xBE800000, 0x3E000000, neg1, 0x3F800000)
    return out


def named_chains():
    """every hand-built chain, in a fixed order"""
    rng = np.random.default_rng(441)
    out = []
    # values: every distribution at every length, carried as chains of eight and five windows
    for name, gen in DISTRIBUTIONS:
        ws = [gen(rng, n) for n in LENGTHS]
        out.append(Chain(name + "_a", ws[:8]))
        out.append(Chain(name + "_b", ws[8:]))
        out.append(Chain(name + "_100", [gen(rng, 100) for _ in range(4)]))
    sp_ = special_middles(rng)
    for name, w in sp_:
        out.append(Chain(name, [w]))
    for k in range(0, len(sp_), 8):                         # ... and what the next window inherits from them
        out.append(Chain("special_chain_%d" % k, [w for _, w in sp_[k:k + 8]]))

    # checkpoints: `copies` of the median key, its nearest neighbours d keys away on each side, no hint
    for tag, sp in (("16", 1 << 16), ("12", 1 << 12), ("8", 1 << 8)):
        smaller = {"16": "12", "12": "8"}.get(tag)
        for d in (sp - 1, sp, sp + 1):
            for low16 in (0x0000, 0xFFFF, 0x5A5A):          # bottom, top and inside of the aligned intervals
                for n in (99, 100, 5, 64):
                    for copies, pos in ((1, 0), (2, 0), (2, 1), (3, 0), (3, 2), (4, 0), (4, 3), (5, 1), (5, 4)):
                        K = K_ONE + 0x10000 + low16
                        kt = (n - 1) >> 1
                        if kt - pos < 1 or n - (kt - pos) - copies < 1:
                            continue                        # no room for a neighbour on each side
                        w = around(n, [K] * copies, rng, d, d, pos)
                        # K at the bottom (top) of its aligned interval of every size: the neighbour above (below) is inside
                        # iff it is less than the size away, so the select leaves at the largest size <= d
                        leave = tag if d >= sp else smaller
                        if low16 == 0x5A5A:
                            want = {"hint_none"}             # inside the intervals: the exit is predict()'s to say
                        elif copies in (2, 3) or leave is None:
                            want = {"hint_none", "bit_0"}    # two or three copies are neither alone nor a crowd
                        else:
                            want = {"hint_none", ("one_" if copies == 1 else "crowd_") + leave}
                        out.append(Chain("checkpoint_%s_d%d_low%04x_n%d_c%d_pos%d" % (tag, d, low16, n, copies, pos), [w], 0,
                                         [want]))
    for copies in (2, 3):                                    # a neighbour one key away: to bit 0
        for n in (100, 99, 4):
            for side in ("lo", "hi"):
                w = around(n, [K_ONE + 0x777] * copies, rng, 1 if side == "lo" else 1 << 20, 1 if side == "hi" else 1 << 20,
                           copies - 1)
                if w is not None:
                    out.append(Chain("one_key_away_c%d_n%d_%s" % (copies, n, side), [w], 0, [{"hint_none", "bit_0"}]))

    # hints
    bases = [("float", _distinct(rng, 100)), ("float_odd", _distinct(rng, 99)), ("quant", _levels(4)(rng, 100)),
             ("quant_odd", _iq8(1.0 / 128, False)(rng, 99)), ("carrier", _carrier(rng, 100)), ("short", _distinct(rng, 3))]
    P23 = 1 << 23
    for bname, w in bases:
        K = median_ref(w)[1]
        srt = np.sort(key_of(w))
        table = [("zero", 0, "hint_none"), ("K", K, {False: "hint_above", True: "hint_exact"}),
                 ("K-1", K - 1, "hint_above"), ("K+1", K + 1, "hint_below"),
                 ("K-(2^23-1)", K - (P23 - 1), "hint_above"), ("K+(2^23-1)", K + (P23 - 1), "hint_below"),
                 ("K-2^23", K - P23, "hint_refused"), ("K+2^23", K + P23, "hint_below"),
                 ("K-(2^23+1)", K - (P23 + 1), "hint_refused"), ("K+(2^23+1)", K + (P23 + 1), "hint_refused"),
                 ("0x007FFFFF", 0x007FFFFF, "hint_none"), ("0x00800000", 0x00800000, "hint_refused"),
                 ("0xFEFFFFFF", 0xFEFFFFFF, "hint_refused"), ("0xFF000000", 0xFF000000, "hint_none"),
                 ("0xFFFFFFFF", 0xFFFFFFFF, "hint_none"),
                 ("present_below", int(srt[0]), None), ("present_above", int(srt[-1]), None)]
        for hname, h, want in table:
            if isinstance(want, dict):
                want = {q: {v} for q, v in want.items()}
            elif want is not None:
                want = {want}
            out.append(Chain("hint_%s_%s" % (bname, hname), [w], h, [want]))

    # chains
    lv = F32(2.0 ** -12)
    again = np.array([1] * 30 + [2] * 40 + [3] * 30, dtype=F32) * lv          # ranks 49, 50 both hold level 2
    split = np.array([1] * 20 + [2] * 30 + [3] * 50, dtype=F32) * lv          # rank 49 is the last 2, rank 50 the first 3
    out.append(Chain("same_median_again", [rng.permutation(again) for _ in range(4)], 0,
                     [{"hint_none", "crowd_16", "upper_count"}] +
                     [{False: {"hint_above", "upper_count"}, True: {"hint_exact", "upper_exact_again"}}] * 3))
    out.append(Chain("same_median_not_again", [rng.permutation(split) for _ in range(4)], 0,
                     [{"hint_none", "crowd_16", "upper_next"}] +
                     [{False: {"hint_above", "upper_next"}, True: {"hint_exact", "upper_next"}}] * 3))
    out.append(Chain("same_median_odd", [rng.permutation(again)[:99] for _ in range(3)], 0,
                     [{"hint_none", "upper_odd"}] + [{False: {"hint_above", "upper_odd"}, True: {"hint_exact", "upper_odd"}}] * 2))
    base = _distinct(rng, 100)
    out.append(Chain("slow_drift", [rng.permutation(base) * F32(1.0 + 0.01 * k) for k in range(8)], 0,
                     [{"hint_none"}] + [{"hint_above"}] * 7))
    out.append(Chain("slow_drift_down", [rng.permutation(base) * F32(1.0 - 0.01 * k) for k in range(8)], 0,
                     [{"hint_none"}] + [{"hint_below"}] * 7))
    out.append(Chain("far_jump", [base, base * F32(1.0e6), base, base * F32(1.0e-6), -base], 0,
                     [{"hint_none"}] + [{"hint_refused"}] * 4))
    empty = np.zeros(0, dtype=F32)
    out.append(Chain("empty_in_the_middle", [base, empty, base, base], 0,
                     [{"hint_none"}, {"hint_refused"}, {"hint_none"}, {False: {"hint_above"}, True: {"hint_exact"}}]))
    nanw = base.copy()
    nanw[17] = np.nan
    out.append(Chain("nan_in_the_middle", [base, nanw, base, nanw], 0, None))
    neg_nans = base.copy()
    neg_nans[:60] = f32(0xFFC00000)                          # the lower middle is itself a (negative) NaN: key 0x003FFFFF
    out.append(Chain("negative_nan_majority", [base, neg_nans, base], 0, [{"hint_none"}, {"hint_refused"}, {"hint_none"}]))
    pos_nans = base.copy()
    pos_nans[:60] = f32(0x7FC00000)                          # ... a positive NaN: key 0xFFC00000, no hint for the next window
    out.append(Chain("positive_nan_majority", [base, pos_nans, base], 0, [{"hint_none"}, {"hint_refused"}, {"hint_none"}]))
    return out


def random_chains(quant, count=4096):
    """`count` chains that mix the distributions above around a per-chain noise floor, for one instance"""
    rng = np.random.default_rng(4096 + (1 if quant else 0))
    gens = [g for _, g in DISTRIBUTIONS]
    out = []
    for c in range(count):
        with np.errstate(all="ignore"):
            out.append(_random_chain(rng, gens, c))
    return out


def _random_chain(rng, gens, c):
    nwins = int(rng.integers(1, 9))
    style = int(rng.integers(0, 6))
    gen = gens[int(rng.integers(0, len(gens)))]
    ws = []
    for k in range(nwins):
        n = int(LENGTHS[rng.integers(0, len(LENGTHS))]) if rng.random() < 0.5 else int(rng.integers(0, 101))
        if rng.random() < 0.7:
            n = (100, 99, 98, 66)[int(rng.integers(0, 4))]
        if style == 0:                                   # one distribution, the floor drifting
            w = gen(rng, n) * F32(1.0 + 0.02 * k)
        elif style == 1:                                 # another distribution every window
            w = gens[int(rng.integers(0, len(gens)))](rng, n)
        elif style == 2:                                 # few copies of the median with near neighbours
            K = K_ONE + int(rng.integers(0, 1 << 18))
            w = around(n, [K] * int(rng.integers(1, 6)), rng, int(2 ** rng.uniform(0, 18)), int(2 ** rng.uniform(0, 18)), 0)
            if w is None:
                w = gen(rng, n)
        elif style == 3:                                 # random bit patterns, NaNs and infinities among them
            w = f32(rng.integers(0, 1 << 32, n))
        elif style == 4:                                 # quantised, the same floor
            w = _levels(int(rng.integers(2, 9)))(rng, n)
        else:                                            # keys within 2^24 of one another: the hint's edge
            w = unkey(K_ONE + rng.integers(0, 1 << 24, n))
        ws.append(w)
    h = int(rng.integers(0, 4))
    K = median_ref(ws[0])[1]
    hint0 = (0, int(rng.integers(0, 1 << 32)), K, K + int(rng.integers(-(1 << 23) - 2, (1 << 23) + 3)))[h]
    return Chain("random_%d" % c, ws, hint0)


def pack(chains):
    """-> (windows float32[total][128], nwin int32[total], chain_start int32[n_chains + 1], hint0 uint32[n_chains])"""
    total = sum(len(c.windows) for c in chains)
    windows = np.zeros((total, WIN), dtype=F32)
    nwin = np.zeros(total, dtype=np.int32)
    start = np.zeros(len(chains) + 1, dtype=np.int32)
    hint0 = np.zeros(len(chains), dtype=U32)
    k = 0
    for c, ch in enumerate(chains):
        start[c] = k
        hint0[c] = ch.hint0
        for w in ch.windows:
            windows[k, :len(w)] = w
            nwin[k] = len(w)
            k += 1
    start[len(chains)] = k
    return windows, nwin, start, hint0


def reference(chains):
    """-> (median bits uint32[total], lower-middle key uint32[total], hint seen by each window uint32[total])"""
    med, key, hint = [], [], []
    for ch in chains:
        h = ch.hint0
        for w in ch.windows:
            m, k = median_ref(w)
            med.append(m)
            key.append(k)
            hint.append(h)
            h = k
    return np.array(med, dtype=U32), np.array(key, dtype=U32), np.array(hint, dtype=U32)


_cache = {}


def all_chains(quant):
    """named + random chains of one instance, with their packed arrays and reference: built once per process"""
    if quant not in _cache:
        if "named" not in _cache:
            _cache["named"] = named_chains()
        chains = _cache["named"] + random_chains(quant)
        _cache[quant] = (chains, pack(chains), reference(chains))
    return _cache[quant]
