"""Record tests/golden/g_merge.npz: one UNMODIFIED reference decoder per receiver stream over per-stream PDU lists that share
their aircraft, under the four (msg_filter, error_corr) configurations, and the ONE table the streams' final plane_dicts fold
into by adsb_stream_planes_merged's rule (include/adsb_hip.h MERGED PICTURE) -- computed here in plain Python from the
reference's dicts, for two selections and two cutoffs.  Container-only tool (tools/ref_harness.py loads the reference by
path); the tests read the .npz alone.

The decoder module's `time` is the PDU clock of tools/make_golden_decode.py (time() = the current PDU's timestamp), so
last_seen = int(timestamp); every stream's clock is the same wall clock.

  bits, ts, stream                     the PDUs in time order; stream: whose list a PDU belongs to (a stream's PDUs keep their order)
  n_streams, sel_0 (empty: every stream), sel_1, cutoffs[2]
  f_<k>_<tag>, f_stream_<tag>          every stream's final plane_dict, one entry per plane in plane_dict's order: icao cs csset
                                       alt altset speed heading vrate vrset lat lon nmsgs seen as in tests/golden/g_expire.npz;
                                       an entry the reference files under "" is stored with icao -1 and takes no part
  m_<k>_<tag>, m_case_<tag>            the merged table of case 2 * selection + cutoff, ascending address: the same fields with
                                       seen = the largest last_seen, and nstreams, src (callsign, altitude, velocity, position)
The rule: a contributing entry is a selected stream's entry with last_seen >= cutoff; num_msgs is the sum modulo 2^32; each
group (callsign: not None; altitude: not NaN; velocity: vertical_rate not NaN -- speed, heading and vertical_rate together;
position: latitude not NaN -- with longitude) is the one of the contributing entry that has it and has the greatest last_seen,
the lowest stream among equals.

The cases (asserted by tests/test_merge.py test_golden_holds_the_cases from the file alone): W's callsign, altitude, velocity
and position each from another stream; X's last_seen tie between streams 1 and 2; Y's velocity, which only its oldest entry
has; Z, whose velocity the cutoff takes away with the entry that held it while a fresher entry keeps the aircraft (a cutoff
hides from the old end, so it cannot hide the freshest entry and keep an older one: this is the case that exists); 0x000000,
in exactly one stream and hidden entirely by the cutoff; 0xFFFFFF in two streams."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_decode as G          # noqa: E402
import make_golden_planes as P          # noqa: E402
import ref_harness as R                 # noqa: E402

W_, X_, Y_, Z_, LO_, HI_ = 0x4B1A01, 0x3C65A2, 0xA0F003, 0x71BC04, 0x000000, 0xFFFFFF
N_STREAMS = 5
T0 = 1760000000.25
CUT = int(T0) + 8
SEL_1 = [1, 3, 4]
INT64_MIN = -(1 << 63)


def flip(b, i):
    b = np.array(b, np.uint8)
    b[i] ^= 1
    return b


def lists(rng):
    """[(stream, seconds after T0, bits)]"""
    s = []

    def at(stream, t, b):
        s.append((stream, T0 + t, np.asarray(b, np.uint8)))
    lat, lon = 47.1, 8.5
    # W: the callsign from stream 0, the altitude from 1, the velocity from 2, the position from 3
    at(3, 5.0, G.position(W_, 0, *G.cpr_encode(lat, lon, 0), alt12=0xC38))
    at(3, 6.0, G.position(W_, 1, *G.cpr_encode(lat, lon, 1), alt12=0xC38))             # a fix: altitude and position, second 6
    at(0, 10.0, G.ident(W_, [1, 2, 3, 4, 5, 6, 7, 8]))
    at(2, 15.0, G.velocity(W_, 1, 0, 300, 1, 120, 0, 9))
    at(1, 20.0, G.position(W_, 0, *G.cpr_encode(lat, lon, 0), alt12=0xD38))             # no fix: another altitude, second 20
    at(1, 20.5, G.df11(W_, rng))
    at(1, 21.0, G.ap_fields(4, W_, rng, ac13=0x0B98))                                  # "All Messages": an AC13 altitude, second 21
    # X: streams 1 and 2 heard it last in the same second
    at(1, 30.1, G.ident(X_, [1, 1, 1, 1, 32, 32, 32, 32]))
    at(2, 30.5, G.ident(X_, [2, 2, 2, 2, 32, 32, 32, 32]))
    at(2, 30.7, G.velocity(X_, 1, 1, 5, 1, 7, 1, 2))
    # Y: only the oldest entry has a velocity; a reply with one wrong bit that "Conservative" repairs
    at(0, 2.0, G.velocity(Y_, 2, 1, 10, 0, 20, 1, 3))
    at(1, 40.0, G.ident(Y_, [3] * 8))
    at(4, 50.0, G.ident(Y_, [4] * 8))
    at(4, 52.0, flip(G.ident(Y_, [9] * 8), 50))
    # Z: the cutoff takes stream 0's entry, and the velocity with it
    at(0, 3.0, G.ident(Z_, [5] * 8))
    at(0, 4.0, G.velocity(Z_, 1, 0, 200, 0, 100, 0, 17))
    at(3, 60.0, G.ident(Z_, [6] * 8))
    # the ends of the address space: 0 in exactly one stream, behind the cutoff
    at(2, 1.0, G.ident(LO_, [7] * 8))
    at(0, 6.2, G.position(HI_, 0, *G.cpr_encode(-33.9, 151.2, 0), alt12=0x5B8))
    at(0, 7.1, G.position(HI_, 1, *G.cpr_encode(-33.9, 151.2, 1), alt12=0x5B8))
    at(4, 45.0, G.ident(HI_, [8] * 8))
    at(4, 45.5, G.df11(HI_, rng))
    at(2, 46.0, rng.integers(0, 2, 112).astype(np.uint8))                              # noise
    s.sort(key=lambda e: e[1])
    return s


KEYS = ("icao", "cs", "csset", "alt", "altset", "speed", "heading", "vrate", "vrset", "lat", "lon", "nmsgs", "seen")
DT = {"icao": np.int32, "cs": np.uint8, "csset": np.int8, "alt": np.int32, "altset": np.int8, "speed": np.uint64, "heading": np.uint64,
      "vrate": np.int32, "vrset": np.int8, "lat": np.uint64, "lon": np.uint64, "nmsgs": np.int64, "seen": np.int64}


def put(out, icao, p, seen):
    out["icao"].append(icao)
    cs = p["callsign"]
    out["cs"].append(np.frombuffer((cs or "").encode().ljust(8, b"\0"), np.uint8))
    out["csset"].append(cs is not None)
    for name, flag, key in (("alt", "altset", "altitude"), ("vrate", "vrset", "vertical_rate")):
        out[flag].append(not P.isnan(p[key]))
        out[name].append(p[key] if out[flag][-1] else 0)
    for name, key in (("speed", "speed"), ("heading", "heading"), ("lat", "latitude"), ("lon", "longitude")):
        out[name].append(G.f64bits(p[key]))
    out["nmsgs"].append(p["num_msgs"])
    out["seen"].append(seen)


def merge(dicts, sel, cutoff):
    """The rule, over the reference's plane_dicts -> [(address, entry, last_seen, n_streams, (src x 4))], ascending address"""
    nan = float("nan")
    groups = (("callsign",), ("altitude",), ("speed", "heading", "vertical_rate"), ("latitude", "longitude"))
    has = (lambda p: p["callsign"] is not None, lambda p: not P.isnan(p["altitude"]), lambda p: not P.isnan(p["vertical_rate"]),
           lambda p: not P.isnan(p["latitude"]))
    table = {}
    for s in sel:
        for key, p in dicts[s].items():
            if key == "" or p["last_seen"] < cutoff:
                continue
            a = int(key, 16)
            m = table.setdefault(a, {"e": {"callsign": None, "altitude": nan, "speed": nan, "heading": nan, "vertical_rate": nan,
                                           "latitude": nan, "longitude": nan, "num_msgs": 0},
                                     "seen": None, "n": 0, "src": [-1] * 4, "t": [None] * 4})
            m["n"] += 1
            m["e"]["num_msgs"] = (m["e"]["num_msgs"] + p["num_msgs"]) % (1 << 32)
            if m["seen"] is None or p["last_seen"] > m["seen"]:
                m["seen"] = p["last_seen"]
            for g in range(4):
                if has[g](p) and (m["src"][g] < 0 or p["last_seen"] > m["t"][g]):
                    for k in groups[g]:
                        m["e"][k] = p[k]
                    m["src"][g], m["t"][g] = s, p["last_seen"]
    return [(a, m["e"], m["seen"], m["n"], m["src"]) for a, m in sorted(table.items())]


def main():
    rng = np.random.default_rng(20261101)
    pdus = lists(rng)
    res = {"bits": np.packbits(np.array([b for _, _, b in pdus], np.uint8), axis=1),
           "ts": np.array([t for _, t, _ in pdus], np.float64), "stream": np.array([s for s, _, _ in pdus], np.int32),
           "n_streams": np.int32(N_STREAMS), "sel_0": np.zeros(0, np.int32), "sel_1": np.array(SEL_1, np.int32),
           "cutoffs": np.array([INT64_MIN, CUT], np.int64)}
    for tag, filt, corr in G.CONFIGS:
        decs = [R.load_reference_decoder(filt, corr, "None") for _ in range(N_STREAMS)]
        clock = G.Clock()
        for s, t, b in pdus:
            dec = decs[s]
            dec.decode_packet.__func__.__globals__["time"] = clock
            clock.now = float(t)
            try:
                dec.decode_packet(({"timestamp": float(t), "snr": 10.0}, np.array(b, np.uint8)))
            except Exception:
                pass
        final = {k: [] for k in KEYS + ("stream",)}
        blanks = [sum(1 for k in d.plane_dict if k == "") for d in decs]
        assert max(blanks) <= (1 if corr == "Conservative" else 0), (tag, blanks)
        for s, d in enumerate(decs):
            for key, p in d.plane_dict.items():
                put(final, int(key, 16) if key != "" else -1, p, p["last_seen"])
                final["stream"].append(s)
        for k in KEYS:
            res["f_%s_%s" % (k, tag)] = np.array(final[k], dtype=DT[k]).reshape((len(final[k]), 8) if k == "cs" else (len(final[k]),))
        res["f_stream_" + tag] = np.array(final["stream"], np.int32)
        merged = {k: [] for k in KEYS + ("nstreams", "src", "case")}
        dicts = [d.plane_dict for d in decs]
        for si, sel in enumerate((list(range(N_STREAMS)), SEL_1)):
            for ci, cutoff in enumerate((INT64_MIN, CUT)):
                for a, e, seen, n, src in merge(dicts, sel, cutoff):
                    put(merged, a, e, seen)
                    merged["nstreams"].append(n)
                    merged["src"].append(src)
                    merged["case"].append(2 * si + ci)
        for k in KEYS:
            res["m_%s_%s" % (k, tag)] = np.array(merged[k], dtype=DT[k]).reshape((len(merged[k]), 8) if k == "cs" else (len(merged[k]),))
        res["m_nstreams_" + tag] = np.array(merged["nstreams"], np.int32)
        res["m_src_" + tag] = np.array(merged["src"], np.int32).reshape(-1, 4)
        res["m_case_" + tag] = np.array(merged["case"], np.int32)
        print(tag, "planes per stream", [len(d.plane_dict) for d in decs], "merged rows per case",
              np.bincount(res["m_case_" + tag], minlength=4).tolist(), "entries under \"\"", blanks)
    path = os.path.join(ROOT, "tests", "golden", "g_merge.npz")
    np.savez_compressed(path, **res)
    print(path, len(pdus), "pdus in", N_STREAMS, "streams", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
