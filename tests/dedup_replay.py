"""The expectation of a shared decoder with ADSB_FLAG_STREAM_DEDUP in plain Python: the rule of include/adsb_hip.h
(DE-DUPLICATION) and its carry around tests/shared_replay.py's Replay -- ONE decoder fed the publication sequence with the
duplicates left out.  Test infrastructure only (tests/test_dedup.py, tests/test_gpu_dedup.py, tools/make_golden_dedup.py)."""
import os

import numpy as np

import aircraft_replay as A
import shared_replay as SR
from gr_adsb_amd import _native as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_dedup.npz")
DUP_NONE, DUP_EARLIER = -1, -2


def payload(b14, fec):
    """(length in bits, the payload's bytes) of a PDU as the decode step receives it: with `fec`, a DF 11/17/18/19 reply whose
    Conservative repair keeps format and length is the repaired reply (ADSB_BURST_FEC_FIXED); 112 bits for the long formats,
    else the first 56 only."""
    bits = A._bits(b14)
    df = A._field(bits, 0, 5)
    L = 112 if df in A.LONG_DFS else 56
    if fec and df in A.PI_DFS and A._mod(bits, L, 24) != 0:
        r = A._repair(bits, L)
        if r is not None:
            df2 = A._field(r, 0, 5)
            if df2 in A.PI_DFS and (df2 in A.LONG_DFS) == (L == 112):
                bits = r
    return L, np.packbits(bits[:L]).tobytes()


def record_payload(rec):
    """The same from a delivered record: its bits are already the repaired ones, its ADSB_BURST_LONG flag the length."""
    L = 112 if int(rec["flags"]) & N.BURST_LONG else 56
    return L, bytes(rec["bits"][:L // 8])


def find_duplicates(pay, ts, stream, carry, window):
    """THE RULE for one call.  pay[t]: a payload, or None for a record that takes no part; carry: [(ts, payload, stream)] of
    earlier calls.  -> (dup[n], the publication order)"""
    n = len(pay)
    order = SR.time_order(ts)
    dup = np.full(n, DUP_NONE, np.int32)
    for k, t in enumerate(order):
        if pay[t] is None:
            continue

        def matches(q_ts, q_pay, q_stream):
            return q_pay == pay[t] and q_stream != stream[t] and abs(float(ts[t]) - float(q_ts)) <= window
        if any(matches(*q) for q in carry):
            dup[t] = DUP_EARLIER
            continue
        for q in order[:k]:
            if pay[q] is not None and matches(ts[q], pay[q], stream[q]):
                dup[t] = q
                break
    return dup, order


def dup_row(b14):
    """The row of a duplicate: that of a record without a PDU over the same bits, port = DEC_DUPLICATE."""
    r = np.zeros(1, dtype=N.DECODED_DTYPE)
    r["port"], r["df"], r["icao"], r["bits"] = N.DEC_DUPLICATE, int(b14[0]) >> 3, -1, np.asarray(b14, np.uint8)
    r["latitude"] = r["longitude"] = np.nan
    return r[0]


class Replay:
    """shared_replay.Replay behind the rule: call() -> (flags, rows, order, dup); rows[t] is None for a record that publishes
    nothing (no PDU, or a duplicate)."""

    def __init__(self, filt, corr, window=0.002, horizon=1.0):
        self.rep = SR.Replay(filt, corr)
        self.fec = corr == "Conservative"
        self.window, self.horizon = float(window), float(horizon)
        self.fresh()

    def fresh(self):
        self.carry, self.hi, self.duplicates = [], 0.0, 0

    def reset(self):
        self.rep.reset()
        self.fresh()

    def call(self, bits14, ts, stream, dem=None, pay=None):
        """pay: the payloads, where the caller has them from delivered records (None: from bits14 by payload())"""
        n = len(bits14)
        dem = np.ones(n, bool) if dem is None else np.asarray(dem, bool)
        if pay is None:
            pay = [payload(bits14[t], self.fec) if dem[t] else None for t in range(n)]
        dup, order = find_duplicates(pay, ts, stream, self.carry, self.window)
        flags, rows, order2 = self.rep.call(bits14, ts, dem=dem & (dup == DUP_NONE))
        assert np.array_equal(order, order2)
        if n:
            self.carry += [(float(ts[t]), pay[t], int(stream[t])) for t in range(n)]
            self.hi = max(q[0] for q in self.carry)
            self.carry = sorted((q for q in self.carry if q[0] >= self.hi - self.horizon), key=lambda q: q[0])
            self.duplicates += int((dup != DUP_NONE).sum())
        return flags, rows, order, dup

    def stats(self):
        return self.duplicates, len(self.carry), self.hi


def received_bits(b14, fec):
    """The 14 bytes the decode step receives: the payload, and behind a short one the raw bytes 7..13."""
    L, p = payload(b14, fec)
    return np.frombuffer(p + bytes(np.asarray(b14, np.uint8)[L // 8:14]), np.uint8)


def rows_of(replayed, bits14, dup, fec=False):
    """Replay.call's rows as DECODED_DTYPE at list positions: the decoder's, a duplicate's dup_row; rows of records without a
    PDU are left zero (the callers compare those apart)."""
    import decode_streams as S
    out = np.zeros(len(replayed), dtype=N.DECODED_DTYPE)
    pub = [t for t, r in enumerate(replayed) if r is not None]
    if pub:
        out[pub] = S.to_rows([replayed[t] for t in pub])
    for t in np.flatnonzero(dup != DUP_NONE):
        out[t] = dup_row(received_bits(bits14[t], fec))
    return out
