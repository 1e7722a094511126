"""A NumPy restatement of the aircraft table (ADSB_FLAG_AIRCRAFT_TABLE; the decoder's plane_dict as check_parity uses it,
decoder.py:576-665), independent of the C helper: the per-PDU rule and a replay of a published sequence.  Used by
tests/test_aircraft.py against tests/golden/g_aircraft.npz and the emulated kernels, and by tests/test_gpu_aircraft.py as
the expected flags of the device."""
import numpy as np

G = 0x1FFF409
AP_DFS = (0, 4, 5, 16, 20, 21, 24)
PI_DFS = (11, 17, 18, 19)
LONG_DFS = (16, 17, 18, 19, 20, 21, 24)
BURST_DEMOD, BURST_AP_FEC, BURST_AP_KNOWN = 1, 0x4, 0x8


def _bits(b14):
    return np.unpackbits(np.asarray(b14, dtype=np.uint8)[:14])


def _mod(bits, L, reg_bits):
    """bits[0:L] as a polynomial mod G (reg_bits 24) or mod x*G (25) -- compute_crc / compute_crc_2."""
    poly = G if reg_bits == 24 else G << 1
    top = 1 << (reg_bits if reg_bits == 24 else 25)
    v = 0
    for x in bits[:L]:
        v = (v << 1) | int(x)
        if v & top:
            v ^= poly
    return v


def _field(bits, lo, n):
    v = 0
    for x in bits[lo:lo + n]:
        v = (v << 1) | int(x)
    return v


_KEYS = {}


def _patterns(L):
    """{25-bit key: (first bit, width)} of the decoder's 1-bit and 2-adjacent-bit patterns (decoder.py:304-323)."""
    if L not in _KEYS:
        t = {}
        for w in (1, 2):
            for i in range(L - w + 1):
                e = np.zeros(L, np.uint8)
                e[i:i + w] = 1
                t[_mod(e, L, 25)] = (i, w)
        _KEYS[L] = t
    return _KEYS[L]


def _repair(bits, L):
    hit = _patterns(L).get(_mod(bits, L, 25))
    if hit is None:
        return None
    r = bits.copy()
    r[hit[0]:hit[0] + hit[1]] ^= 1
    return r


def announce(bits):
    """The address a passing reply announces through update_plane (DF 11; 17/18/19 by CF/AF and TC/ST), or -1."""
    df, sub, tc, st = _field(bits, 0, 5), _field(bits, 5, 3), _field(bits, 32, 5), _field(bits, 37, 3)
    aa = _field(bits, 8, 24)
    if df == 11:
        return aa
    if df == 17 or (df == 18 and sub in (0, 1, 6)) or (df == 19 and sub == 0):
        if 1 <= tc <= 4 or 9 <= tc <= 18 or (tc == 19 and st in (1, 2)):
            return aa
    return -1


_RULES = {}


def rule(b14, fec):
    """(aa, announce, rep, fec_announce) of one payload: see adsb_mode_s_aircraft."""
    key = (bytes(np.asarray(b14, dtype=np.uint8)[:14]), bool(fec))
    if key not in _RULES:
        _RULES[key] = _rule(_bits(b14), fec)
    return _RULES[key]


def _rule(bits, fec):
    df = _field(bits, 0, 5)
    L = 112 if df in LONG_DFS else 56
    aa, ann, rep, fann = -1, -1, False, -1
    if df in AP_DFS:
        aa = _mod(bits, L, 24)
        r = _repair(bits, L) if fec else None
        if r is not None:
            rep = True
            df2 = _field(r, 0, 5)
            fann = aa if (df2 in AP_DFS and df2 != 24) else announce(r)
    elif df in PI_DFS:
        if _mod(bits, L, 24) == 0:
            ann = announce(bits)
        elif fec:
            r = _repair(bits, L)
            if r is not None:
                ann = announce(r)
    return aa, ann, rep, fann


def _pi_passes(b14, fec):
    bits = _bits(b14)
    L = 56 if _field(bits, 0, 5) == 11 else 112
    return _mod(bits, L, 24) == 0 or (fec and _repair(bits, L) is not None)


def replay(b14s, fec, table=None):
    """A published sequence through one decoder: -> (flags, added, passed), one entry per PDU.  flags: BURST_AP_KNOWN /
    BURST_AP_FEC as the device sets them; added: the address the PDU adds to the table (-1: none); passed: the decoder
    (msg_filter "All Messages") accepts it.  table: a set of known addresses, updated in place (several calls)."""
    known = set() if table is None else table
    flags, added, passed = [], [], []
    for b in b14s:
        aa, ann, rep, fann = rule(b, fec)
        f, new, ok = 0, -1, False
        if aa >= 0:
            if aa in known:
                f, ok = BURST_AP_KNOWN, True
            elif rep:
                f, ok = BURST_AP_FEC, True
                new = fann
        elif (int(b[0]) >> 3) in PI_DFS:
            ok = _pi_passes(b, fec)
            new = ann
        if new >= 0 and new not in known:
            known.add(new)
        else:
            new = -1
        flags.append(f)
        added.append(new)
        passed.append(ok)
    return np.array(flags, np.uint16), np.array(added, np.int64), np.array(passed, bool)


def expected_records(recs, fec, table):
    """What a FLAG_AIRCRAFT_TABLE context makes of one pass's records (as a flag-off context delivers them, after k_fec):
    the replay's BURST_AP_KNOWN / BURST_AP_FEC added to the records with BURST_DEMOD, in list order; table: the set of
    known addresses, carried from pass to pass."""
    out = recs.copy()
    dem = np.nonzero((recs["flags"] & BURST_DEMOD) != 0)[0]
    fl, _, _ = replay(recs["bits"][dem], fec, table)
    out["flags"][dem] |= fl
    return out
