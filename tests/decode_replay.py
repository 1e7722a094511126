"""A plain-Python restatement of the decoder's message decoding as ADSB_FLAG_DECODE folds it (decode_packet, decode_message,
decode_me, the CPR global decode, update_plane; decoder.py:330-1512), independent of the reference and of the device code.
It turns a published sequence into the rows the device writes (include/adsb_hip.h adsb_decoded): used by tests/test_decode.py
against tests/golden/g_decode.npz and the emulated kernels, and by tests/test_gpu_decode.py as the expected rows.

Clock: now = int(timestamp) of the PDU being decoded (the decoder's int(time.time()) in real time with zero latency)."""
import math

import numpy as np

import aircraft_replay as AR

NONE, DECODED, UNKNOWN, RAISED = 0, 1, 2, 3
HAS_PLANE, HAS_CALLSIGN, HAS_ALTITUDE, HAS_VELOCITY = 1, 2, 4, 8
CALLSIGN_LUT = "_ABCDEFGHIJKLMNOPQRSTUVWXYZ_____ _______________0123456789______"
NL_EDGES = [10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686,
            31.77209708, 33.53993436, 35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012,
            44.19454951, 45.54626723, 46.86733252, 48.16039128, 49.42776439, 50.67150166, 51.89342469, 53.09516153,
            54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277, 61.04917774, 62.13216659,
            63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
            71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083,
            79.29428225, 80.24923213, 81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621,
            86.53536998, 87.00000000]
NAN = float("nan")


def nl(lat):
    lat = -lat if lat < 0 else lat
    for k, e in enumerate(NL_EDGES):
        if lat < e:
            return 59 - k
    return 1


def cpr_global(e, o):
    """(lat, lon) of an even frame e and an odd frame o, each (lat_cpr, lon_cpr, t); NaN when their zones differ.  The
    frames' ages are checked by the caller."""
    late, lone, lato, lono = e[0] / 131072, e[1] / 131072, o[0] / 131072, o[1] / 131072
    j = math.floor(59 * late - 60 * lato + 0.5)
    lat_even = 360.0 / 60 * ((j % 60) + late)
    if lat_even >= 270:
        lat_even -= 360
    lat_odd = 360.0 / 59 * ((j % 59) + lato)
    if lat_odd >= 270:
        lat_odd -= 360
    if nl(lat_even) != nl(lat_odd):
        return NAN, NAN
    if e[2] - o[2] > 0:
        lat, frame, base = lat_even, 0, lone
    else:
        lat, frame, base = lat_odd, 1, lono
    n = nl(lat)
    ni = max(n - frame, 1)
    m = math.floor(lone * (n - 1) - lono * n + 0.5)
    lon = (360.0 / ni) * ((m % ni) + base)
    if lon >= 180.0:
        lon -= 360.0
    return lat, lon


def ac13(v):
    if v == 0 or (v >> 6) & 1 or not (v >> 4) & 1:
        return -1
    n = ((v >> 7) << 5) | (((v >> 5) & 1) << 4) | (v & 0xF)      # bits 6 (M) and 8 (Q) removed
    return n * 25 - 1000


def ac12(v):
    if not (v >> 4) & 1:
        return -1
    return (((v >> 5) << 4) | (v & 0xF)) * 25 - 1000


def f(bits, lo, n):
    return AR._field(bits, lo, n)


def classify(b14, msg_filter_all, fec, known):
    """One published PDU before the fold: (accepted bits or None, the decoder's bits after the PDU, filed address or -1).
    known(aa): the address is in the table."""
    raw = AR._bits(b14)
    df = f(raw, 0, 5)
    L = 112 if df in AR.LONG_DFS else 56
    if df in AR.AP_DFS:
        if not msg_filter_all:
            return None, raw, -1
        aa = AR._mod(raw, L, 24)
        if known(aa):
            return raw, raw, aa
        r = AR._repair(raw, L) if fec else None
        if r is None:
            return None, raw, aa
        return r, r, aa
    if df in AR.PI_DFS and (msg_filter_all or df != 11):
        if AR._mod(raw, L, 24) == 0:
            return raw, raw, -1
        r = AR._repair(raw, L) if fec else None
        if r is not None:
            return r, r, -1
    return None, raw, -1


def event(bits, aa, msg_filter_all):
    """(kind, filed address, port) of an accepted PDU: kind 'snap' (no change), 'count', 'alt13', 'ident', 'pos', 'vel'."""
    df = f(bits, 0, 5)
    if msg_filter_all:
        if df in (0, 16, 4, 20):
            return ("alt13" if aa >= 0 else "snap"), aa, NONE
        if df in (5, 21):
            return ("count" if aa >= 0 else "snap"), aa, NONE
        if df == 11:
            return "count", f(bits, 8, 24), NONE
    if df not in (17, 18, 19):
        return "snap", aa, NONE
    a, sub = f(bits, 8, 24), f(bits, 5, 3)
    if df == 18 and sub in (2, 3, 5):
        return "snap", a, RAISED
    if (df == 18 and sub not in (0, 1, 6)) or (df == 19 and sub != 0):
        return "snap", a, NONE
    tc, st = f(bits, 32, 5), f(bits, 37, 3)
    if tc == 0:
        return "snap", a, NONE
    if tc <= 4:
        return "ident", a, DECODED
    if tc <= 8 or tc >= 20:
        return "snap", a, UNKNOWN
    if tc <= 18:
        return "pos", a, NONE
    if st in (1, 2):
        return "vel", a, DECODED
    return "snap", a, (NONE if st in (3, 4) else RAISED)


class Decoder:
    """The fold of one decoder: plane state per address, carried from call to call."""

    def __init__(self, msg_filter="All Messages", error_corr="None"):
        self.all = msg_filter == "All Messages"
        self.fec = error_corr == "Conservative"
        self.planes = {}

    def row(self, b14, ts):
        """One PDU (14 packed bytes, float64 timestamp) -> a dict of the row's fields."""
        now = int(ts)
        acc, after, aa = classify(b14, self.all, self.fec, lambda a: a in self.planes)
        port, kind = NONE, None
        df = f(after, 0, 5)
        if acc is not None:
            kind, aa, port = event(acc, aa, self.all)
        p = self.planes.get(aa) if aa >= 0 else None
        if kind not in (None, "snap"):
            if p is None:
                p = self.planes[aa] = dict(callsign=None, altitude=None, vel=None, lat=NAN, lon=NAN, cpr=[None, None], n=0)
            p["n"] += 1
            if kind == "alt13":
                v = ac13(f(acc, 19, 13))
                if v != -1:
                    p["altitude"] = v
            elif kind == "ident":
                p["callsign"] = "".join(CALLSIGN_LUT[f(acc, 40 + 6 * k, 6)] for k in range(8)).replace("_", "")
            elif kind == "pos":
                odd = int(acc[53])
                p["cpr"][odd] = (f(acc, 54, 17), f(acc, 71, 17), now)
                e, o = p["cpr"]
                lat = lon = NAN
                if e is not None and o is not None and now - e[2] < 30 and now - o[2] < 30:
                    lat, lon = cpr_global(e, o)
                if lat - p["lat"] < 0.1:
                    port = DECODED
                p["altitude"] = ac12(f(acc, 40, 12))
                if not math.isnan(lat) and not math.isnan(lon):
                    p["lat"], p["lon"] = lat, lon
            elif kind == "vel":
                vwe = f(acc, 46, 10) - 1
                vsn = f(acc, 57, 10) - 1
                vr = (f(acc, 69, 9) - 1) * 64
                p["vel"] = (-vwe if acc[45] else vwe, -vsn if acc[56] else vsn, -vr if acc[68] else vr)
        r = dict(port=port, df=df, icao=aa, bits=np.packbits(after), present=0, callsign=b"", altitude=0, vwe=0, vsn=0, vrate=0,
                 lat=NAN, lon=NAN, num_msgs=0)
        if p is not None:
            r["present"] = HAS_PLANE
            if p["callsign"] is not None:
                r["present"] |= HAS_CALLSIGN
                r["callsign"] = p["callsign"].encode()
            if p["altitude"] is not None:
                r["present"] |= HAS_ALTITUDE
                r["altitude"] = p["altitude"]
            if p["vel"] is not None:
                r["present"] |= HAS_VELOCITY
                r["vwe"], r["vsn"], r["vrate"] = p["vel"]
            r["lat"], r["lon"], r["num_msgs"] = p["lat"], p["lon"], p["n"]
        return r

    def rows(self, b14s, tss):
        return [self.row(b, t) for b, t in zip(b14s, tss)]


def f64bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def speed_heading(vwe, vsn):
    """What the reference derives from the integer components (decoder.py:1190-1191)."""
    return np.sqrt(vsn**2 + vwe**2), np.arctan2(vsn, vwe) * 360.0 / (2.0 * np.pi)
