"""PDU streams for the ADSB_FLAG_DECODE tests: mixed traffic of given aircraft (positions in even / odd pairs, identifications,
velocities, address/parity replies, DF 11, noise) with float64 timestamps, and a row comparison that reports the first
difference.  Test infrastructure only."""
import math

import numpy as np

import decode_replay as D
from gr_adsb_amd import _native as N
from gr_adsb_amd import modulator as M


def ib(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def es(aa, tc, body, df=17, sub=0):
    f = np.zeros(112, np.uint8)
    f[:5], f[5:8], f[8:32], f[32:37], f[37:88] = ib(df, 5), ib(sub, 3), ib(aa, 24), ib(tc, 5), body
    f[88:] = ib(M.crc24(f[:88]), 24)
    return f


def ap(df, aa, rng):
    L = 56 if df in (0, 4, 5) else 112
    f = np.zeros(112, np.uint8)
    f[:5] = ib(df, 5)
    f[5:L - 24] = rng.integers(0, 2, L - 29)
    f[L - 24:L] = ib(M.crc24(f[:L - 24]) ^ aa, 24)
    if L == 56:
        f[56:] = rng.integers(0, 2, 56)
    return f


def cpr_encode(lat, lon, odd):
    dlat = 360.0 / (60 - odd)
    yz = math.floor(131072 * (lat % dlat) / dlat + 0.5)
    rlat = dlat * (yz / 131072 + math.floor(lat / dlat))
    dlon = 360.0 / max(D.nl(rlat) - odd, 1)
    xz = math.floor(131072 * (lon % dlon) / dlon + 0.5)
    return int(yz) % 131072, int(xz) % 131072


def message(rng, aa, state):
    """One PDU of aircraft aa (state: its track), 112 bits."""
    kind = int(rng.integers(0, 12))
    if kind < 6:
        state["lat"] += state["vlat"]
        state["lon"] += state["vlon"]
        la, lo = cpr_encode(state["lat"], state["lon"], state["odd"])
        body = np.zeros(51, np.uint8)
        body[3:15], body[16], body[17:34], body[34:51] = ib(int(rng.integers(0, 4096)), 12), state["odd"], ib(la, 17), ib(lo, 17)
        state["odd"] ^= 1
        return es(aa, int(rng.integers(9, 19)), body)
    if kind == 6:
        body = np.zeros(51, np.uint8)
        for k in range(8):
            body[3 + 6 * k:9 + 6 * k] = ib(int(rng.integers(0, 64)), 6)
        return es(aa, int(rng.integers(1, 5)), body)
    if kind == 7:
        body = rng.integers(0, 2, 51).astype(np.uint8)
        body[:3] = ib(int(rng.integers(1, 3)), 3)
        return es(aa, 19, body)
    if kind in (8, 9):
        return ap(int(rng.choice([0, 4, 5, 16, 20, 21, 24])), aa, rng)
    if kind == 10:
        f = np.zeros(112, np.uint8)
        f[:5], f[5:8], f[8:32] = ib(11, 5), ib(5, 3), ib(aa, 24)
        f[32:56] = ib(M.crc24(f[:32]), 24)
        return f
    f = rng.integers(0, 2, 112).astype(np.uint8)
    if rng.integers(0, 2):                     # a damaged reply: one or two adjacent bits flipped
        f = es(aa, int(rng.integers(0, 32)), rng.integers(0, 2, 51).astype(np.uint8))
        i = int(rng.integers(0, 111))
        f[i:i + int(rng.integers(1, 3))] ^= 1
    return f


def mixed(rng, n, addresses, t0=1760000000.5, dt=(0.002, 0.4)):
    """n PDUs of the given aircraft: (bits14 [n, 14], timestamps [n])."""
    states = {a: dict(lat=float(rng.uniform(-80, 80)), lon=float(rng.uniform(-179, 179)), vlat=float(rng.uniform(-0.002, 0.002)),
                      vlon=float(rng.uniform(-0.002, 0.002)), odd=int(rng.integers(0, 2))) for a in addresses}
    b, ts, t = [], [], t0
    order = list(addresses) + [int(x) for x in rng.choice(addresses, max(0, n - len(addresses)))]
    for a in order[:n]:
        t += float(rng.uniform(*dt))
        b.append(np.packbits(message(rng, a, states[a])))
        ts.append(t)
    return np.array(b, np.uint8), np.array(ts, np.float64)


def to_rows(rs):
    """decode_replay rows (dicts) -> DECODED_DTYPE."""
    out = np.zeros(len(rs), dtype=N.DECODED_DTYPE)
    for i, r in enumerate(rs):
        out[i] = (r["port"], r["df"], r["present"], 0, r["icao"], r["bits"], r["callsign"], (0, 0), r["altitude"], r["vwe"],
                  r["vsn"], r["vrate"], r["lat"], r["lon"], r["num_msgs"], 0)
    return out


def assert_rows_equal(got, exp):
    """DECODED_DTYPE rows byte for byte (exp may be decode_replay dicts)."""
    if not isinstance(exp, np.ndarray):
        exp = to_rows(exp)
    assert len(got) == len(exp), (len(got), len(exp))
    g, e = got.view(np.uint8).reshape(len(got), -1), exp.view(np.uint8).reshape(len(exp), -1)
    bad = np.flatnonzero(np.any(g != e, axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]], exp[bad[:2]])
