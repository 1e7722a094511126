"""The expectation of a shared decoder (ADSB_FLAG_STREAM_DECODE_SHARED) in plain Python: ONE tests/decode_replay.py decoder and
ONE tests/aircraft_replay.py table fed every call's PDUs in the order ascending (timestamp, list position), and the call
partitions of tests/golden/g_shared.npz.  Test infrastructure only (tests/test_shared_decode.py, tools/shared_sanitize_job.py)."""
import os

import numpy as np

import aircraft_replay as A
import decode_replay as D
import decode_streams as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_shared.npz")


def time_order(ts):
    return np.array(sorted(range(len(ts)), key=lambda t: (ts[t], t)), np.int64)


def time_key_np(ts):
    """The monotone map k_shared_keys and the de-duplication step state (time_key), in NumPy: ascending keys <=> ascending
    doubles -- a set sign bit flips every bit, a clear one sets it -- and -0.0 takes +0.0's key."""
    b = np.ascontiguousarray(ts, dtype=np.float64).view(np.uint64).copy()
    b[b == np.uint64(1 << 63)] = 0
    return np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))


class Replay:
    """ONE decode_replay.Decoder and ONE aircraft_replay table fed every call in the order (ts, t); results at list positions,
    with plane_dict's last_seen kept beside the planes."""

    def __init__(self, filt, corr):
        self.cfg = (filt, corr)
        self.reset()

    def reset(self):
        self.dec, self.known, self.seen = D.Decoder(*self.cfg), set(), {}

    def call(self, bits14, ts, dem=None):
        n = len(bits14)
        order = time_order(ts)
        rows = [None] * n
        flags = np.zeros(n, np.uint16)
        pub = [t for t in order if dem is None or dem[t]]
        if pub:
            flags[pub] = A.replay(bits14[pub], self.dec.fec, self.known)[0]
        for t in pub:
            before = {a: p["n"] for a, p in self.dec.planes.items()}
            rows[t] = self.dec.row(bits14[t], ts[t])
            for a, p in self.dec.planes.items():
                if before.get(a) != p["n"]:
                    self.seen[a] = int(ts[t])
        return flags, rows, order

    def expire(self, cutoff):
        gone = [a for a, t in self.seen.items() if t < cutoff]
        for a in gone:
            del self.dec.planes[a], self.seen[a]
            self.known.discard(a)
        return len(gone)


def rows_of(replayed):
    return S.to_rows([r for r in replayed if r is not None])


def golden_calls(g, partition):
    """[(list positions, extra empty items)]: partition 0 the file's calls; 1: every call cut in two at its median timestamp,
    which keeps the publication sequence (equal timestamps stay together)."""
    out = []
    for c in range(int(g["call"].max()) + 1):
        idx = np.flatnonzero(g["call"] == c)
        present = set(g["stream"][idx].tolist())
        items = g["items_%d" % c].tolist()
        extra = [(k, s) for k, s in enumerate(items) if s not in present]
        if partition == 0:
            out.append((idx, extra))
        else:
            mid = np.median(g["ts"][idx])
            lo, hi = idx[g["ts"][idx] < mid], idx[g["ts"][idx] >= mid]
            out += [(lo, []), (hi, [])]
    return [(i, e) for i, e in out if len(i)]
