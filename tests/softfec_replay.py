"""The soft-decision CRC repair (include/adsb_hip.h: SOFT REPAIR) restated in plain Python / NumPy: what the kernels of
gr_adsb_amd/csrc/adsb_softfec_device.h and the host rule adsb_mode_s_soft_fec are held against, byte for byte.  Test
infrastructure only; nothing here calls the library."""
import itertools

import numpy as np

G = 0x1FFF409
PI_DFS = (11, 17, 18, 19)
LONG_DFS = (16, 17, 18, 19, 20, 21, 24)
SHORT_DFS = (0, 4, 5, 11)
DEMOD, PARITY_OK, LONG, KNOWN_DF, DF_SHIFT, FEC_FIXED, FEC_DF = 1, 32, 64, 128, 8, 0x4000, 0x8000
SOFT_DTYPE = np.dtype([("nflip", "u1"), ("ncand", "u1"), ("bit", "u1", (5,)), ("pad", "u1")])
REC_DTYPE = np.dtype([("offset", "<i8"), ("peak", "<f4"), ("median", "<f4"), ("bits", "u1", (14,)), ("flags", "<u2")])
DEFAULTS = dict(n_weak=8, max_flips=3, min_key=0.0)


def rem_tab():
    r, v = [], 1
    for _ in range(112):
        r.append(v)
        v <<= 1
        if v & 0x1000000:
            v ^= G
    return r


R = rem_tab()        # R[j] = x^j mod G; bit i of an L-bit reply contributes R[L-1-i]


def unpack(bits14):
    return np.unpackbits(np.asarray(bits14, dtype=np.uint8).reshape(14), bitorder="big")


def pack(bits112):
    return np.packbits(np.asarray(bits112, dtype=np.uint8).reshape(112), bitorder="big")


def df_of(bits):
    return int(bits[0]) * 16 + int(bits[1]) * 8 + int(bits[2]) * 4 + int(bits[3]) * 2 + int(bits[4])


def length_of(df):
    return 112 if df in LONG_DFS else 56


def syndrome(bits, L):
    s = 0
    for i in range(L):
        if bits[i]:
            s ^= R[L - 1 - i]
    return s


def prefilter_flags(bits):
    """the pre-filter bits of a demodulated record's flags, from its 112 bits"""
    df = df_of(bits)
    f = df << DF_SHIFT
    if df in LONG_DFS:
        f |= LONG
    if df in LONG_DFS or df in SHORT_DFS:
        f |= KNOWN_DF
    if df in PI_DFS and syndrome(bits, length_of(df)) == 0:
        f |= PARITY_OK
    return f


def keys(x1, x0):
    """weakness of every bit from its two float32 samples: lo / hi by the slicer's own comparison, ONE float32 division"""
    x1, x0 = np.asarray(x1, dtype=np.float32), np.asarray(x0, dtype=np.float32)
    first = x1 > x0
    hi, lo = np.where(first, x1, x0), np.where(first, x0, x1)
    good = (hi > 0) & (lo >= 0) & (hi < np.float32(np.inf))
    with np.errstate(all="ignore"):
        q = (lo / hi).astype(np.float32)
    return np.where(good, q, np.where(~(hi > 0), np.float32(1.0), np.float32(0.0))).astype(np.float32)


def candidates(key, L, n_weak, min_key):
    cand = [i for i in range(5, L) if key[i] >= np.float32(min_key)]
    cand.sort(key=lambda i: (-float(key[i]), i))
    return cand[:n_weak]


def search(S, cand, L, max_flips):
    """-> (flips, mask) of the best matching subset or None: fewest flips, then the smallest mask (mask bit k = rank k)"""
    best = None
    for k in range(1, min(max_flips, len(cand)) + 1):
        for sub in itertools.combinations(range(len(cand)), k):
            s = 0
            for r in sub:
                s ^= R[L - 1 - cand[r]]
            if s == S:
                m = sum(1 << r for r in sub)
                if best is None or (k, m) < best:
                    best = (k, m)
        if best is not None:
            break
    return best


def row_of(nflip, ncand, flipped):
    row = np.zeros((), dtype=SOFT_DTYPE)
    row["nflip"], row["ncand"] = nflip, ncand
    row["bit"] = (sorted(flipped) + [0xFF] * 5)[:5]
    return row


def soft_rule(bits, key, n_weak=8, max_flips=3, min_key=0.0):
    """One reply (112 bits 0/1, key[112]): -> (bits after the rule, repaired?, row).  The caller has checked DEMOD / FEC_DF;
    this checks the DF and the syndrome."""
    bits = np.array(bits, dtype=np.uint8)
    df = df_of(bits)
    if df not in PI_DFS:
        return bits, False, np.zeros((), dtype=SOFT_DTYPE)
    L = length_of(df)
    S = syndrome(bits, L)
    if S == 0:
        return bits, False, np.zeros((), dtype=SOFT_DTYPE)
    cand = candidates(key, L, n_weak, min_key)
    best = search(S, cand, L, max_flips)
    if best is None:
        return bits, False, row_of(0, len(cand), [])
    flipped = [cand[r] for r in range(len(cand)) if best[1] >> r & 1]
    bits[flipped] ^= 1
    return bits, True, row_of(best[0], len(cand), flipped)


def conservative(bits, L):
    """the Conservative table's pattern for an L-bit reply (1 bit / 2 adjacent bits, keyed by syndrome and last bit) or None"""
    S = syndrome(bits, L)
    for j in range(L):
        if R[j] == S and bits[L - 1] == (1 if j == 0 else 0):
            return [L - 1 - j]
    for j in range(1, L):
        if R[j] ^ R[j - 1] == S and bits[L - 1] == (1 if j == 1 else 0):
            return [L - 1 - j, L - j]
    return None


def conservative_record(bits, flags):
    """fec_record: -> (bits, flags) of a record after the Conservative repair"""
    bits = np.array(bits, dtype=np.uint8)
    df = df_of(bits)
    if not (flags & DEMOD) or (flags & PARITY_OK) or df not in PI_DFS:
        return bits, flags
    L = length_of(df)
    pat = conservative(bits, L)
    if pat is None:
        return bits, flags
    fixed = bits.copy()
    fixed[pat] ^= 1
    df2 = df_of(fixed)
    if df2 in PI_DFS and length_of(df2) == L:
        keep = flags & ~(PARITY_OK | LONG | KNOWN_DF | (31 << DF_SHIFT))
        return fixed, keep | prefilter_flags(fixed) | FEC_FIXED
    return bits, flags | FEC_DF


def sample_keys(x, p, sps):
    """keys of the 112 bits of the burst at local index p of the float32 |IQ|^2 stream x (zero outside it, as the device reads)"""
    x = np.asarray(x, dtype=np.float32)
    i1 = p + 8 * sps + np.arange(112, dtype=np.int64) * sps
    i0 = i1 + sps // 2

    def at(i):
        ok = (i >= 0) & (i < len(x))
        return np.where(ok, x[np.where(ok, i, 0)], np.float32(0.0)).astype(np.float32)
    return keys(at(i1), at(i0))


def replay_records(recs, x, origin, sps, rule=None, with_conservative=False):
    """The records of a pass (REC_DTYPE, raw: as a context without any repair delivers them) over the converted samples x
    (float32 |IQ|^2, local index 0 = stream offset origin) -> (records, SOFT_DTYPE rows) as a FLAG_FEC_SOFT context delivers
    them (with_conservative: | FLAG_FEC_CONSERVATIVE)."""
    rule = dict(DEFAULTS, **(rule or {}))
    out = np.array(recs, dtype=REC_DTYPE)
    rows = np.zeros(len(out), dtype=SOFT_DTYPE)
    for t in range(len(out)):
        fl = int(out["flags"][t])
        bits = unpack(out["bits"][t])
        if with_conservative:
            bits, fl = conservative_record(bits, fl)
        if (fl & DEMOD) and not (fl & (PARITY_OK | FEC_DF)) and df_of(bits) in PI_DFS:
            key = sample_keys(x, int(out["offset"][t]) - origin, sps)
            bits, fixed, rows[t] = soft_rule(bits, key, **rule)
            if fixed:
                keep = fl & ~(PARITY_OK | LONG | KNOWN_DF | (31 << DF_SHIFT))
                fl = keep | prefilter_flags(bits) | FEC_FIXED
        out["bits"][t] = pack(bits)
        out["flags"][t] = fl
    return out, rows


def replay_slices(bits14, ok, tag_idx, x, sps, rule=None):
    """adsb_demod_work's slices (packed bits [n,14], ok bytes, local tag positions) -> (bits14, ok, rows) after the soft repair"""
    rule = dict(DEFAULTS, **(rule or {}))
    bits14, ok = np.array(bits14, dtype=np.uint8).reshape(-1, 14), np.array(ok, dtype=np.uint8)
    rows = np.zeros(len(ok), dtype=SOFT_DTYPE)
    for t in range(len(ok)):
        fl = int(ok[t])
        bits = unpack(bits14[t])
        if (fl & DEMOD) and not (fl & (PARITY_OK | (FEC_DF >> 13))) and df_of(bits) in PI_DFS:
            bits, fixed, rows[t] = soft_rule(bits, sample_keys(x, int(tag_idx[t]), sps), **rule)
            if fixed:
                bits14[t] = pack(bits)
                ok[t] = (fl & 1) | (prefilter_flags(bits) & 0xE0) | (FEC_FIXED >> 13)
    return bits14, ok, rows
