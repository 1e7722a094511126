"""Container-only: generate tests/golden/g_decode.npz and tests/golden/g_decode_edges.npz -- known answers of the REFERENCE decoder's message decoding
(decoder.py:330-352 decode_packet, :883-1060 decode_message, :1065-1301 decode_me, :1309-1512 the CPR global decode, :413-440
update_plane, :512-538 the published PDUs) for sequences of PDUs, under msg_filter "All Messages" / "Extended Squitter Only"
and error_corr "None" / "Conservative".  Data only: inputs (packed bits, timestamps, snr, sequence ids) and the reference's
outputs.

The decoder's clock: the reference ages CPR frames with int(time.time()).  Here the decoder module's `time` is a clock that
returns the current PDU's timestamp, so now = int(meta["timestamp"]) -- what the reference computes when it decodes in
real time with zero latency, and the clock the device step defines (include/adsb_hip.h ADSB_FLAG_DECODE).

Each sequence goes to a fresh decoder, one PDU after the other.  The sequences: every sequence of tools/make_golden_aircraft.py
(every DF/CF/AF/TC/ST class, address/parity replies around their announcements, Conservative repairs of AP replies into
DF 17/18/19, DF 11/17/19 replies whose repair changes the format, noise, mixed traffic), then all 64 callsign codes, AC13
and AC12 in every Q/M case, CPR pairs in every NL zone of both hemispheres, pairs whose latitudes fall in different zones,
the frame choice (even newer, same second, odd newer), frame ages of 29/30/31 s, the signed 0.1 degree publish test,
position messages without a fix, velocity signs and zero fields, and a long mixed sequence of a few aircraft.

Outputs per configuration <m>_<e> (m: all / es, e: none / cons), one entry per PDU:
  port_*      0 nothing published, 1 "decoded", 2 "unknown", 3 decode_packet raised
  pfix_*      the decoder's self.bits after the PDU (its repair applied), packed, XOR the input bits: pbits = bits ^ pfix is
              what a published PDU carries
  df_*, icao_*  self.df; int(self.aa_str, 16), -1 for ""
  has_*       plane_dict[aa_str] exists after the PDU (aa_str "" never counts: it is not an address)
  the snapshot of plane_dict[aa_str] (zero / NaN when has_ == 0):
  cs_*        callsign bytes (8, NUL padded); csset_*: callsign is not None
  alt_*, altset_*  altitude (int) and whether it is not NaN
  speed_*, heading_*  float64 bits; vrate_*, vrset_*: vertical_rate (int), not NaN
  lat_*, lon_*  float64 bits; nmsgs_*: num_msgs
  types_*     for published "decoded" PDUs: type codes of callsign, altitude, speed, heading, vertical_rate, latitude,
              longitude, num_msgs (0 None, 1 int, 2 float, 3 numpy.float64, 4 str)
Shared: datetime (the published "datetime" string of every PDU), keys_decoded / keys_unknown (the published dicts' keys).

g_decode_edges.npz has the same fields for the sequences of edge_sequences: CPR pairs on the latitude grid points next to each
of the 58 NL zone edges in both hemispheres with either frame the newer one, pairs whose frames lie on different sides of an
edge, |latitude| >= 87, latitude 0, longitudes on each side of 180 and CPR latitudes around the 270 wrap.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_aircraft as A            # noqa: E402
import ref_harness as R                     # noqa: E402
from gr_adsb_amd import modulator as M      # noqa: E402

CONFIGS = A.CONFIGS
ib = A.ib
T0 = 1760000000.25


def es(df, aa, tc, body, sub=0):
    """A DF 17/18/19 reply with parity: ME = tc (5 bits) + body (51 bits)."""
    f = np.zeros(112, np.uint8)
    f[:5] = ib(df, 5)
    f[5:8] = ib(sub, 3)
    f[8:32] = ib(aa, 24)
    f[32:37] = ib(tc, 5)
    f[37:88] = body
    f[88:] = ib(M.crc24(f[:88]), 24)
    return f


def ident(aa, codes, tc=4):
    body = np.zeros(51, np.uint8)
    body[:3] = ib(5, 3)
    for k, c in enumerate(codes):
        body[3 + 6 * k:9 + 6 * k] = ib(c, 6)
    return es(17, aa, tc, body)


def position(aa, odd, lat_cpr, lon_cpr, alt12=0xC38, tc=11, df=17, sub=0):
    body = np.zeros(51, np.uint8)
    body[3:15] = ib(alt12, 12)          # bits 40..51
    body[15] = 0                         # T, bit 52
    body[16] = odd                       # F, bit 53
    body[17:34] = ib(lat_cpr, 17)
    body[34:51] = ib(lon_cpr, 17)
    return es(df, aa, tc, body, sub)


def velocity(aa, st, sew, vew, sns, vns, svr, vr, src=0):
    body = np.zeros(51, np.uint8)
    body[:3] = ib(st, 3)                 # bits 37..39
    body[8] = sew                        # bit 45
    body[9:19] = ib(vew, 10)             # 46..55
    body[19] = sns                       # 56
    body[20:30] = ib(vns, 10)            # 57..66
    body[30] = src                       # 67
    body[31] = svr                       # 68
    body[32:41] = ib(vr, 9)              # 69..77
    return es(17, aa, 19, body)


def ap_fields(df, aa, rng, ac13=None):
    """An address/parity reply of AA `aa` with bits 19..31 = ac13 (random otherwise)."""
    L = 56 if df in (0, 4, 5) else 112
    f = np.zeros(L, np.uint8)
    f[:5] = ib(df, 5)
    f[5:L - 24] = rng.integers(0, 2, L - 29)
    if ac13 is not None:
        f[19:32] = ib(ac13, 13)
    f[L - 24:] = ib(M.crc24(f[:L - 24]) ^ aa, 24)
    return A.pad112(f, rng)


def df11(aa, rng):
    return A.pi_reply(11, aa, rng)


def nl_of(lat):
    if abs(lat) >= 87.0:
        return 1
    nz = 60.0
    return int(2.0 * math.pi / math.acos(1.0 - (1.0 - math.cos(math.pi / (2.0 * nz))) / math.cos(math.pi / 180.0 * abs(lat)) ** 2))


def cpr_encode(lat, lon, odd):
    dlat = 360.0 / (60 - odd)
    yz = math.floor(131072 * (lat % dlat) / dlat + 0.5)
    rlat = dlat * (yz / 131072 + math.floor(lat / dlat))
    dlon = 360.0 / max(nl_of(rlat) - odd, 1)
    xz = math.floor(131072 * (lon % dlon) / dlon + 0.5)
    return int(yz) % 131072, int(xz) % 131072


def pair(aa, lat, lon, t, dt_odd=1.0, alt12=0xC38):
    """(even, odd) position replies of one true position, the even one at t, the odd one at t + dt_odd."""
    e = position(aa, 0, *cpr_encode(lat, lon, 0), alt12=alt12)
    o = position(aa, 1, *cpr_encode(lat, lon, 1), alt12=alt12)
    return [(e, t), (o, t + dt_odd)]


# the NL zone edges of decoder.py:1362-1512
NL_EDGES = [10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686,
            31.77209708, 33.53993436, 35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012,
            44.19454951, 45.54626723, 46.86733252, 48.16039128, 49.42776439, 50.67150166, 51.89342469, 53.09516153,
            54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277, 61.04917774, 62.13216659,
            63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
            71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083,
            79.29428225, 80.24923213, 81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621,
            86.53536998, 87.00000000]


def decode_sequences(rng, addr):
    seqs = []
    t = T0

    def nxt(step=0.37):
        nonlocal t
        t += step
        return t
    # callsigns: every code, an all-"_" callsign (""), spaces, every TC 1-4
    a = next(addr)
    s = [(df11(a, rng), nxt())]
    for k in range(8):
        s.append((ident(a, list(range(8 * k, 8 * k + 8)), tc=1 + k % 4), nxt()))
    s += [(ident(a, [0] * 8), nxt()), (ident(a, [32, 1, 32, 0, 2, 32, 32, 32]), nxt()), (ident(a, [48 + k for k in range(8)]), nxt())]
    seqs.append(s)
    # AC13 in DF 0/4/16/20 (and DF 5/21 counting): zero, M = 1, M = 0 with Q = 0 / 1; a NaN altitude survives -1
    a = next(addr)
    s = [(df11(a, rng), nxt())]
    vals = [0, 1 << 6, (1 << 6) | 0x1FFF & ~(1 << 6), 0x1F3F & ~(1 << 8), 1 << 8, (1 << 8) | 1, 0x1FFF & ~(1 << 6)]
    vals += [int(v) for v in rng.integers(0, 1 << 13, 24)]
    for k, v in enumerate(vals):
        df = (0, 4, 16, 20)[k % 4]
        s.append((ap_fields(df, a, rng, ac13=v), nxt()))
        if k % 5 == 0:
            s.append((ap_fields((5, 21)[k % 2], a, rng), nxt()))
    seqs.append(s)
    # AC12, Q = 0 and 1, in single position frames (no fix: the altitude is still stored, -1 included)
    a = next(addr)
    s = []
    for v in [0, 1 << 4, 0xFFF, 0xFFF & ~(1 << 4), 0x010, 0x011] + [int(x) for x in rng.integers(0, 1 << 12, 10)]:
        s.append((position(a, int(rng.integers(0, 2)), int(rng.integers(0, 131072)), int(rng.integers(0, 131072)), alt12=v), nxt()))
        s.append((ap_fields(4, a, rng, ac13=0), nxt()))
    seqs.append(s)
    # CPR pairs in every NL zone, both hemispheres, longitudes of every sign; both frame orders
    edges = [0.0] + NL_EDGES + [90.0]
    for z in range(len(edges) - 1):
        lo, hi = edges[z], edges[z + 1]
        for hemi in (1, -1):
            a = next(addr)
            lat = hemi * (lo + (hi - lo) * float(rng.uniform(0.2, 0.8)))
            lon = float(rng.uniform(-180, 180))
            t0 = nxt(5.0)
            p = pair(a, lat, lon, t0, dt_odd=float(rng.choice([1.2, -1.2])))
            p.sort(key=lambda x: x[1])
            lat2 = lat + hemi * float(rng.uniform(-0.05, 0.05))
            p += pair(a, lat2, lon + 0.01, t0 + 3.0, dt_odd=1.0)
            seqs.append(p)
    # even / odd frames in different zones (no fix), near the zone edges
    for e in NL_EDGES[::3]:
        a = next(addr)
        t0 = nxt(5.0)
        ev = position(a, 0, *cpr_encode(e - 0.02, 10.0, 0))
        od = position(a, 1, *cpr_encode(e + 0.02, 10.0, 1))
        seqs.append([(ev, t0), (od, t0 + 0.5), (position(a, 0, *cpr_encode(e + 0.02, 10.0, 0)), t0 + 1.5)])
    # random CPR values: every sign of every wrap
    a = next(addr)
    s = []
    for _ in range(60):
        s.append((position(a, int(rng.integers(0, 2)), int(rng.integers(0, 131072)), int(rng.integers(0, 131072))), nxt(0.6)))
    seqs.append(s)
    # frame choice: even newer, same second, odd newer (whole seconds of the PDU timestamps)
    for de, do in ((2.1, 0.3), (0.1, 0.6), (0.3, 2.2), (0.7, 0.2), (1.0, 0.0), (0.0, 1.0)):
        a = next(addr)
        lat, lon = float(rng.uniform(-80, 80)), float(rng.uniform(-180, 180))
        base = math.floor(nxt(10.0))
        seqs.append([(position(a, 1, *cpr_encode(lat, lon, 1)), base + do), (position(a, 0, *cpr_encode(lat, lon, 0)), base + de)]
                    if do < de else
                    [(position(a, 0, *cpr_encode(lat, lon, 0)), base + de), (position(a, 1, *cpr_encode(lat, lon, 1)), base + do)])
    # frame ages 29 / 30 / 31 s, for each frame
    for age in (29, 30, 31):
        for first in (0, 1):
            a = next(addr)
            lat, lon = float(rng.uniform(-80, 80)), float(rng.uniform(-180, 180))
            base = math.floor(nxt(40.0)) + 0.4
            f1 = position(a, first, *cpr_encode(lat, lon, first))
            f2 = position(a, 1 - first, *cpr_encode(lat, lon, 1 - first))
            seqs.append([(f1, base), (f2, base + age + 0.3), (f2, base + age - 0.5), (f1, base + age + 0.1)])
    # the signed 0.1 degree publish test: first fix, small and large negative steps, steps of 0.1 and more
    a = next(addr)
    lat, lon = 45.0, 7.0
    s = []
    for d in (0.0, -0.001, -0.02, -3.0, 0.05, 0.099, 0.1, 0.15, 2.0, -0.0, 0.0999999):
        lat += d
        s += pair(a, lat, lon, nxt(1.0), dt_odd=0.4)
    seqs.append(s)
    # velocities: signs and zero fields, ST 1/2 (3/4 and 0/5/6/7 in the class sequences and below)
    a = next(addr)
    s = [(df11(a, rng), nxt())]
    for st in (1, 2, 3, 4, 0, 5, 6, 7):
        for sew, vew, sns, vns, svr, vr in ((0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 1), (0, 2, 1, 2, 0, 2), (1, 1023, 0, 1023, 1, 511),
                                           (0, 1, 1, 0, 1, 0), (1, 0, 0, 1, 0, 1), (1, 300, 1, 400, 1, 20), (0, 5, 0, 7, 0, 9)):
            s.append((velocity(a, st, sew, vew, sns, vns, svr, vr), nxt()))
    seqs.append(s)
    # a long mixed sequence: a few aircraft over several minutes
    planes = []
    for _ in range(5):
        planes.append(dict(aa=next(addr), lat=float(rng.uniform(-70, 70)), lon=float(rng.uniform(-179, 179)),
                           vlat=float(rng.uniform(-0.003, 0.003)), vlon=float(rng.uniform(-0.003, 0.003)), odd=0))
    s = []
    tm = nxt(1.0)
    for _ in range(900):
        tm += float(rng.uniform(0.05, 0.5))
        p = planes[int(rng.integers(0, len(planes)))]
        p["lat"] += p["vlat"]
        p["lon"] += p["vlon"]
        kind = int(rng.integers(0, 10))
        if kind < 5:
            s.append((position(p["aa"], p["odd"], *cpr_encode(p["lat"], p["lon"], p["odd"]), alt12=int(rng.integers(0, 4096))), tm))
            p["odd"] ^= 1
        elif kind == 5:
            s.append((ident(p["aa"], [int(c) for c in rng.integers(0, 64, 8)], tc=int(rng.integers(1, 5))), tm))
        elif kind == 6:
            s.append((velocity(p["aa"], int(rng.integers(1, 3)), *[int(x) for x in (rng.integers(0, 2), rng.integers(0, 1024),
                                                                                    rng.integers(0, 2), rng.integers(0, 1024),
                                                                                    rng.integers(0, 2), rng.integers(0, 512))]), tm))
        elif kind == 7:
            s.append((ap_fields(int(rng.choice([0, 4, 5, 16, 20, 21])), p["aa"], rng, ac13=int(rng.integers(0, 8192))), tm))
        elif kind == 8:
            s.append((df11(p["aa"], rng), tm))
        else:
            s.append((rng.integers(0, 2, 112).astype(np.uint8), tm))
    seqs.append(s)
    return seqs


# ---- tests/golden/g_decode_edges.npz: the NL zone edges on the CPR latitude grid --------------------------------------------
# A decoded latitude is a grid point: 6 k / 131072 degrees from an even frame, (360 / 59) k / 131072 from an odd one (k < 0 in
# the south).  Around every edge, in both hemispheres, the file holds the fixes of the last grid point below it and of the first
# one at or above it, from each frame, and pairs whose frames lie on different sides (no fix).
DLAT = (360.0 / 60, 360.0 / 59)


def grid_lat(k, odd):
    return DLAT[odd] * (k / 131072)


def grid_below(e, odd):
    """The largest k whose grid latitude is below e (e > 0)."""
    k = int(e / DLAT[odd] * 131072) + 2
    while not grid_lat(k, odd) < e:
        k -= 1
    return k


def table_nl(lat):
    lat = abs(lat)
    for k, e in enumerate(NL_EDGES):
        if lat < e:
            return 59 - k
    return 1


def grid_position(aa, odd, k, lon, alt12):
    """The position reply of frame `odd` at grid latitude index k (signed) and longitude lon."""
    dlon = 360.0 / max(table_nl(grid_lat(k, odd)) - odd, 1)
    xz = math.floor(131072 * (lon % dlon) / dlon + 0.5)
    return position(aa, odd, k % 131072, int(xz) % 131072, alt12=alt12)


def triple(aa, ke, ko, lon, t, rng):
    """Even, odd, even one second apart: after the second reply the odd frame is the newer one, after the third the even."""
    alt = [int(v) | 0x10 for v in rng.integers(0, 4096, 3)]
    return [(grid_position(aa, 0, ke, lon, alt[0]), t), (grid_position(aa, 1, ko, lon, alt[1]), t + 1.0),
            (grid_position(aa, 0, ke, lon + 0.0001, alt[2]), t + 2.0)]


def edge_sequences(rng):
    addr = iter(rng.permutation(np.arange(0x100000, 0xFFFFFF))[:2000].tolist())
    seqs = []
    t = T0
    for e in NL_EDGES:
        be, bo = grid_below(e, 0), grid_below(e, 1)
        for hemi in (1, -1):
            lon = float(rng.uniform(-180, 180))
            for ke, ko in ((be, bo), (be + 1, bo + 1), (be, bo + 1), (be + 1, bo)):     # below, above, two straddles
                t += 7.0
                seqs.append(triple(next(addr), hemi * ke, hemi * ko, lon, t, rng))
    # NL = 1 (ni clamped to 1 for the odd frame), the poles' neighbourhood, latitude 0 and its neighbours
    for lat in (87.5, 89.0, 89.9999, -87.5, -89.0, -89.9999, 0.0, 0.00005, -0.00005):
        for lon in (-170.0, -0.00001, 0.0, 33.0, 179.99999):
            t += 7.0
            ke, ko = int(round(lat / DLAT[0] * 131072)), int(round(lat / DLAT[1] * 131072))
            seqs.append(triple(next(addr), ke, ko, lon, t, rng))
    # longitudes on each side of 180 in many zones
    for lat in (-80.0, -52.3, -10.0, 0.0, 10.0, 33.3, 61.0, 86.0):
        for lon in (179.9999, 179.99999, 180.0, -179.99999, -179.9999, 180.00001):
            t += 7.0
            ke, ko = int(round(lat / DLAT[0] * 131072)), int(round(lat / DLAT[1] * 131072))
            seqs.append(triple(next(addr), ke, ko, lon, t, rng))
    # the 270 wrap of lat_even / lat_odd: CPR latitudes around the south pole's (even 0, odd 32768 with j = -15)
    for yz0 in (131070, 131071, 0, 1, 2):
        for yz1 in (32766, 32767, 32768, 32769, 32770):
            t += 7.0
            a = next(addr)
            xz = [int(v) for v in rng.integers(0, 131072, 3)]
            seqs.append([(position(a, 0, yz0, xz[0]), t), (position(a, 1, yz1, xz[1]), t + 1.0), (position(a, 0, yz0, xz[2]), t + 2.0)])
    return seqs


def all_sequences(rng):
    addr = iter(rng.permutation(np.arange(0x100000, 0xFFFFFF))[:6000].tolist())
    seqs = []
    t = T0 - 50000.0
    for s in A.sequences(rng):               # timestamps for the class and repair sequences: a PDU every 0.3 s
        seqs.append([(b, t + 0.3 * k) for k, b in enumerate(s)])
        t += 0.3 * len(s) + 40.0
    return seqs + decode_sequences(rng, addr)


class Clock:
    """The decoder module's `time`: time() returns the current PDU's timestamp."""
    now = 0.0

    def time(self):
        return self.now


def tcode(v):
    if v is None:
        return 0
    if isinstance(v, str):
        return 4
    if isinstance(v, np.float64):
        return 3
    if isinstance(v, float):
        return 2
    if isinstance(v, int):
        return 1
    raise TypeError(type(v))


def f64bits(v):
    return int(np.array([float(v)], np.float64).view(np.uint64)[0])


def run(dec, rows, out, keys):
    clock = Clock()
    dec.decode_packet.__func__.__globals__["time"] = clock
    for b, ts, snr in rows:
        clock.now = ts
        vec = np.array(b, dtype=np.uint8)
        n0 = len(dec.msgs)
        raised = 0
        try:
            dec.decode_packet(({"timestamp": ts, "snr": snr}, vec))
        except Exception:
            raised = 1
        new = dec.msgs[n0:]
        assert len(new) <= 1 and not (raised and new)
        port = 3 if raised else (0 if not new else {"decoded": 1, "unknown": 2}[new[0][0]])
        if new:
            meta, v = new[0][1]
            assert v is vec
            keys[port] = tuple(meta)
        out["port"].append(port)
        out["pbits"].append(np.packbits(vec))
        out["df"].append(dec.df)
        aa = dec.aa_str
        out["icao"].append(int(aa, 16) if aa != "" else -1)
        p = dec.plane_dict.get(aa) if aa != "" else None
        out["has"].append(p is not None)
        p = p or {"callsign": None, "altitude": np.nan, "speed": np.nan, "heading": np.nan, "vertical_rate": np.nan,
                  "latitude": np.nan, "longitude": np.nan, "num_msgs": 0}
        cs = p["callsign"]
        out["cs"].append(np.frombuffer((cs or "").encode().ljust(8, b"\0"), np.uint8))
        out["csset"].append(cs is not None)
        alt = p["altitude"]
        out["altset"].append(not (isinstance(alt, float) and math.isnan(alt)))
        out["alt"].append(alt if out["altset"][-1] else 0)
        out["speed"].append(f64bits(p["speed"]))
        out["heading"].append(f64bits(p["heading"]))
        vr = p["vertical_rate"]
        out["vrset"].append(not (isinstance(vr, float) and math.isnan(vr)))
        out["vrate"].append(vr if out["vrset"][-1] else 0)
        out["lat"].append(f64bits(p["latitude"]))
        out["lon"].append(f64bits(p["longitude"]))
        out["nmsgs"].append(p["num_msgs"])
        if port == 1:
            m = new[0][1][0]
            out["types"].append([tcode(m[k]) for k in ("callsign", "altitude", "speed", "heading", "vertical_rate",
                                                      "latitude", "longitude", "num_msgs")])
        else:
            out["types"].append([0] * 8)


def emit(seqs, rng, name):
    """Run every sequence through a fresh reference decoder under each configuration and write tests/golden/<name>."""
    rows = [(np.asarray(b, np.uint8), float(ts)) for s in seqs for b, ts in s]
    snr = rng.uniform(0, 40, len(rows)).astype(np.float32)
    bits = np.array([b for b, _ in rows], dtype=np.uint8)
    ts = np.array([t for _, t in rows], dtype=np.float64)
    seq = np.array([i for i, s in enumerate(seqs) for _ in s], dtype=np.int32)
    import datetime
    res = {"bits": np.packbits(bits, axis=1), "ts": ts, "snr": snr, "seq": seq,
           "datetime": np.array([datetime.datetime.utcfromtimestamp(x).strftime("%Y-%m-%d %H:%M:%S.%f UTC") for x in ts])}
    keys = {}
    for tag, filt, corr in CONFIGS:
        out = {k: [] for k in ("port", "pbits", "df", "icao", "has", "cs", "csset", "alt", "altset", "speed", "heading",
                               "vrate", "vrset", "lat", "lon", "nmsgs", "types")}
        k0 = 0
        for s in seqs:
            dec = R.load_reference_decoder(filt, corr, "None")
            run(dec, [(np.asarray(b, np.uint8), float(t), float(snr[k0 + j])) for j, (b, t) in enumerate(s)], out, keys)
            k0 += len(s)
        dt = {"port": np.int8, "pbits": np.uint8, "df": np.int8, "icao": np.int32, "has": np.int8, "cs": np.uint8,
              "csset": np.int8, "alt": np.int32, "altset": np.int8, "speed": np.uint64, "heading": np.uint64, "vrate": np.int32,
              "vrset": np.int8, "lat": np.uint64, "lon": np.uint64, "nmsgs": np.int32, "types": np.uint8}
        for k, v in out.items():
            res["%s_%s" % (k, tag)] = np.array(v, dtype=dt[k])
        res["pfix_" + tag] = res.pop("pbits_" + tag) ^ res["bits"]
        p = res["port_" + tag]
        print(tag, "decoded", int((p == 1).sum()), "unknown", int((p == 2).sum()), "raised", int((p == 3).sum()),
              "planes", len(set(res["icao_" + tag][res["has_" + tag] == 1].tolist())))
    for port, key in ((1, "keys_decoded"), (2, "keys_unknown")):
        if port in keys:
            res[key] = np.array(keys[port])
    path = os.path.join(ROOT, "tests", "golden", name)
    np.savez_compressed(path, **res)
    print(path, len(bits), "pdus in", len(seqs), "sequences", os.path.getsize(path), "bytes")


def main():
    rng = np.random.default_rng(20261017)
    emit(all_sequences(rng), rng, "g_decode.npz")
    rng = np.random.default_rng(20261018)
    emit(edge_sequences(rng), rng, "g_decode_edges.npz")


if __name__ == "__main__":
    main()
