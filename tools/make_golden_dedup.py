"""Record tests/golden/g_dedup.npz: ONE UNMODIFIED reference decoder behind four receiver streams that hear the same replies,
fed the publication sequence of a shared decoder (tools/make_golden_shared.py) WITH THE DUPLICATES LEFT OUT -- the contract of
ADSB_FLAG_STREAM_DEDUP (include/adsb_hip.h DE-DUPLICATION) -- under the four (msg_filter, error_corr) configurations.  The
duplicates are computed here, by the header's rule in plain Python (duplicates() below: no device code, no replay module).
Container-only tool (tools/ref_harness.py loads the reference by path); the tests read the .npz alone.

Stored as g_shared.npz stores it, everything per PDU at the PDU's LIST position:
  fs, start[4], window, horizon         window = 2^-9 s, horizon = 4 s; the starts differ by exactly window (stream 1) and by
                                        window + one representable step (stream 2: an ulp at 1.76e9 is 2^-22 s)
  bits, stream, offset, call, items_<c>, ts, order      as g_shared.npz
  dup_<e>                               e: none / cons -- dup[] of the rule (-1, -2, or a list position OF THE SAME CALL,
                                        counted from the call's first record) for error_corr None / Conservative: the payload
                                        of a repaired reply is the repaired one
  port_<tag> ... nmsgs_<tag>, pfix_<tag>  per PDU what g_shared.npz holds; at a duplicate port = 4 and nothing else
  f_<k>_<tag>                           the final plane_dict
  case_<x>                              list positions of the PDUs the cases are about

The cases (asserted here, and by tests/test_dedup.py from the file alone):
  (a) one DF 17 identification heard by streams 0, 1, 2 within the window: num_msgs 1
  (b) the even CPR frame heard by streams 0 and 2, the odd one by 1 and 3: a position, num_msgs 2
  (c) two hearings whose ts differ by exactly window: a duplicate; a pair one representable step beyond: not one
  (d) the same payload twice on stream 0 inside the window: both published
  (e) a DF 11 whose bytes 7..13 differ between two receivers: a duplicate; a DF 17 that differs in its last byte: not one
  (f) a hearing delivered in a later call with an EARLIER timestamp than the first hearing: dup = -2
  (g) a hearing delivered after hi has moved more than horizon past it: published again
  (h) a DF 4 reply heard twice: the second a duplicate whatever the table says; a DF 11 all-call heard twice: announced once,
      and a later DF 4 to that address is known
  (i) a duplicate whose earliest match in its own call is itself a duplicate of a carry entry: dup = -2"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aircraft_replay as AR            # noqa: E402
import decode_streams as S              # noqa: E402
import make_golden_decode as G          # noqa: E402
import make_golden_merge as MG          # noqa: E402
import ref_harness as R                 # noqa: E402

FS = 2e6
T0 = 1760000000.25
WINDOW, HORIZON, ULP = 2.0 ** -9, 4.0, 2.0 ** -22
START = [T0, T0 + WINDOW, T0 + WINDOW + ULP, T0 - 1.0]
A1, PB, AC1, AC2, AD, AE, AE2, AF, AG, AH, AH2, AI = (0x4B1A01, 0x4B1A02, 0x3C65A1, 0x3C65A2, 0x71BC04, 0x89ABCD, 0x89ABCE, 0xA0F001,
                                                     0xA0F002, 0x500001, 0x500002, 0x500003)
FLEET = [0x400000 + 4099 * k for k in range(10)]
SHARED_FLEET = [0x420000 + 4099 * k for k in range(6)]
ITEMS = [[0, 1, 2, 3], [3, 0, 2], [2, 3, 0, 1], [1]]
N_CALLS = len(ITEMS)
SHORT_DFS = (0, 4, 5, 11)


def offset_of(stream, x):
    """The sample of the common clock's second x on `stream`."""
    return int(round((x - (START[stream] - T0)) * FS))


def events(rng):
    """[(call, stream, offset, packed bits, label)]"""
    ev = []

    def hear(call, stream, x, b, label="", offset=None, tail=None):
        b = np.asarray(b, np.uint8)
        b = (b if len(b) == 112 else np.unpackbits(b)).copy()
        if (int(np.packbits(b[:8])[0]) >> 3) in SHORT_DFS:
            b[56:] = rng.integers(0, 2, 56)                 # every receiver slices its own noise behind a short reply
        if tail is not None:
            b[104:] ^= np.unpackbits(np.array([tail], np.uint8))
        ev.append((call, stream, offset_of(stream, x) if offset is None else offset, np.packbits(b), label))
    # every stream's own traffic, and traffic that streams 0, 1 and sometimes 2 share: stream 1 hears it 0.4 ms or 3.5 ms later
    for s in range(4):
        b, t = S.mixed(np.random.default_rng(700 + s), n=40, addresses=FLEET, t0=0.0, dt=(0.05, 1.2))
        x = np.round(t / t[-1] * 9.3 * 1e4) / 1e4 + 0.05013
        for k in range(len(b)):
            hear(0, s, float(x[k]), b[k])
    b, t = S.mixed(np.random.default_rng(710), n=36, addresses=SHARED_FLEET, t0=0.0, dt=(0.05, 1.2))
    x = np.round(t / t[-1] * 9.3 * 1e4) / 1e4 + 0.07517
    for k in range(len(b)):
        hear(0, 0, float(x[k]), b[k], "bg")
        hear(0, 1, float(x[k]) + (0.0004 if k % 2 == 0 else 0.0035), b[k], "bg_dup" if k % 2 == 0 else "bg_far")
        if k % 3 == 0:
            hear(0, 2, float(x[k]) + 0.0011, b[k], "bg_dup")
    lat, lon = 47.1, 8.5
    ident = G.ident(A1, [1, 2, 3, 4, 5, 6, 7, 8])
    for s, d, lab in ((0, 0.0, "a0"), (1, 0.0003, "a1"), (2, 0.0007, "a2")):
        hear(0, s, 2.0 + d, ident, lab)
    even, odd = G.position(PB, 0, *G.cpr_encode(lat, lon, 0)), G.position(PB, 1, *G.cpr_encode(lat, lon, 1))
    hear(0, 0, 3.0, even, "b_e0"), hear(0, 2, 3.0004, even, "b_e1")
    hear(0, 1, 4.0, odd, "b_o0"), hear(0, 3, 4.0005, odd, "b_o1")
    o = int(5.0 * FS)
    c1, c2 = G.ident(AC1, [3] * 8), G.ident(AC2, [4] * 8)
    hear(0, 0, 0, c1, "c_q", offset=o), hear(0, 1, 0, c1, "c_dup", offset=o)
    hear(0, 0, 0, c2, "c_q2", offset=o + 4000), hear(0, 2, 0, c2, "c_not", offset=o + 4000)
    d = G.ident(AD, [5] * 8)
    hear(0, 0, 6.0, d, "d0"), hear(0, 0, 6.0005, d, "d1")
    e = G.df11(AE, rng)
    hear(0, 0, 7.0, e, "e_q"), hear(0, 1, 7.0002, e, "e_dup")
    e2 = G.ident(AE2, [6] * 8)
    hear(0, 0, 7.5, e2, "e_q2"), hear(0, 1, 7.5002, e2, "e_not", tail=0x55)
    f = G.ident(AF, [7] * 8)
    hear(0, 0, 9.9995, f, "f_q"), hear(1, 3, 9.9990, f, "f_dup")
    g = G.ident(AG, [8] * 8)
    hear(1, 0, 12.0, g, "g_q"), hear(3, 1, 12.0005, g, "g_again")
    h = G.ap_fields(4, AH, rng, ac13=0x0B98)
    hear(1, 0, 13.0, h, "h_q"), hear(1, 2, 13.0003, h, "h_dup")
    h2 = G.df11(AH2, rng)
    hear(1, 0, 13.5, h2, "h_ann"), hear(1, 2, 13.5003, h2, "h_ann_dup")
    hear(1, 0, 14.0, G.ap_fields(4, AH2, rng, ac13=0x0B98), "h_known")
    i = G.ident(AI, [9] * 8)
    hear(1, 0, 15.0, i, "i_q"), hear(2, 2, 15.0003, i, "i_dup1"), hear(2, 3, 15.0006, i, "i_dup2")
    # call 2 moves hi past 12 + horizon; a reply that a Conservative decoder repairs, heard clean by another receiver
    b, t = S.mixed(np.random.default_rng(720), n=12, addresses=FLEET, t0=0.0, dt=(0.05, 0.3))
    for k in range(len(b)):
        hear(2, 0, 16.0 + float(np.round(t[k] / t[-1] * 2.0, 4)), b[k])
    fx = G.ident(A1, [9] * 8)
    hear(2, 0, 18.5, fx, "fec_q"), hear(2, 2, 18.5004, MG.flip(fx, 50), "fec_dup")
    return ev


def payload(b14, fec):
    """The header's payload: (length, bytes) -- the repaired reply where ADSB_BURST_FEC_FIXED would be set."""
    bits = np.unpackbits(np.asarray(b14, np.uint8))
    df = int(b14[0]) >> 3
    L = 112 if df in AR.LONG_DFS else 56
    if fec and df in AR.PI_DFS and AR._mod(bits, L, 24) != 0:
        r = AR._repair(bits, L)
        if r is not None and (int(np.packbits(r[:8])[0]) >> 3) in AR.PI_DFS and ((int(np.packbits(r[:8])[0]) >> 3) in AR.LONG_DFS) == (L == 112):
            bits = r
    return L, np.packbits(bits[:L]).tobytes()


def duplicates(bits, ts, stream, call, order, fec):
    """THE RULE over the whole publication sequence: -> dup[] (a list position of the whole file, -2, or -1).  A record of an
    earlier call is held iff its ts >= hi - horizon with hi over all calls before r's."""
    n = len(ts)
    pay = [payload(bits[t], fec) for t in range(n)]
    dup = np.full(n, -1, np.int64)
    for k, r in enumerate(order):
        earlier = [t for t in range(n) if call[t] < call[r]]
        hi = max((ts[t] for t in earlier), default=0.0)
        for q in order[:k]:
            if call[q] < call[r] and not ts[q] >= hi - HORIZON:
                continue
            if stream[q] != stream[r] and pay[q] == pay[r] and abs(float(ts[r]) - float(ts[q])) <= WINDOW:
                if call[q] < call[r]:
                    dup[r] = -2
                    break
                if dup[r] == -1:
                    dup[r] = q
    return dup


def main():
    rng = np.random.default_rng(20270115)
    ev = events(rng)
    rows = []
    for c in range(N_CALLS):
        for s in ITEMS[c]:
            rows += sorted((e for e in ev if e[0] == c and e[1] == s), key=lambda e: e[2])
    n = len(rows)
    assert n == len(ev)
    call = np.array([r[0] for r in rows], np.int32)
    stream = np.array([r[1] for r in rows], np.int32)
    offset = np.array([r[2] for r in rows], np.int64)
    bits = np.array([r[3] for r in rows], np.uint8)
    start = np.array(START, np.float64)
    ts = start[stream] + offset.astype(np.float64) / FS
    for s in range(4):
        assert np.all(np.diff(offset[stream == s]) > 0), s          # a stream's records are in stream order, call after call
    order = np.concatenate([np.array(sorted(np.flatnonzero(call == c).tolist(), key=lambda t: (ts[t], t)), np.int64) for c in range(N_CALLS)])
    pos = {r[4]: k for k, r in enumerate(rows) if r[4] and not r[4].startswith("bg")}
    labels = np.array([r[4] for r in rows])
    res = {"fs": np.float64(FS), "start": start, "window": np.float64(WINDOW), "horizon": np.float64(HORIZON), "bits": bits,
           "stream": stream, "offset": offset, "call": call, "ts": ts, "order": order.astype(np.int32)}
    for c in range(N_CALLS):
        res["items_%d" % c] = np.array(ITEMS[c], np.int32)
    first_of_call = np.array([np.flatnonzero(call == c)[0] for c in range(N_CALLS)])
    dups = {}
    for e, fec in (("none", False), ("cons", True)):
        d = duplicates(bits, ts, stream, call, order, fec)
        dups[e] = d
        # the cases are what they claim to be
        assert d[pos["a0"]] == -1 and d[pos["a1"]] == pos["a0"] and d[pos["a2"]] == pos["a0"]
        assert [d[pos[k]] for k in ("b_e0", "b_e1", "b_o0", "b_o1")] == [-1, pos["b_e0"], -1, pos["b_o0"]]
        assert ts[pos["c_dup"]] - ts[pos["c_q"]] == WINDOW and d[pos["c_dup"]] == pos["c_q"]
        assert ts[pos["c_not"]] - ts[pos["c_q2"]] == WINDOW + ULP and np.nextafter(WINDOW, 1) < WINDOW + ULP and d[pos["c_not"]] == -1
        assert np.nextafter(ts[pos["c_q2"]] + WINDOW, np.inf) == ts[pos["c_not"]]          # one representable step
        assert d[pos["d0"]] == d[pos["d1"]] == -1 and ts[pos["d1"]] - ts[pos["d0"]] <= WINDOW
        assert d[pos["e_dup"]] == pos["e_q"] and not np.array_equal(bits[pos["e_dup"]][7:], bits[pos["e_q"]][7:])
        assert d[pos["e_not"]] == -1 and np.array_equal(bits[pos["e_not"]][:13], bits[pos["e_q2"]][:13])
        assert d[pos["f_dup"]] == -2 and call[pos["f_dup"]] > call[pos["f_q"]] and ts[pos["f_dup"]] < ts[pos["f_q"]]
        assert d[pos["g_again"]] == -1 and ts[call < 3].max() - ts[pos["g_q"]] > HORIZON and abs(ts[pos["g_again"]] - ts[pos["g_q"]]) <= WINDOW
        assert d[pos["h_dup"]] == pos["h_q"] and d[pos["h_ann_dup"]] == pos["h_ann"] and d[pos["h_known"]] == -1
        assert d[pos["i_dup1"]] == -2 and d[pos["i_dup2"]] == -2 and call[pos["i_dup1"]] == call[pos["i_dup2"]]
        assert d[pos["fec_dup"]] == (pos["fec_q"] if fec else -1)
        assert all(d[t] >= 0 for t in np.flatnonzero(labels == "bg_dup")) and all(d[t] == -1 for t in np.flatnonzero(labels == "bg_far"))
        rel = d.copy()
        rel[d >= 0] -= first_of_call[call[d >= 0]]
        assert all(call[d[t]] == call[t] for t in np.flatnonzero(d >= 0))
        res["dup_" + e] = rel.astype(np.int32)
    for k, v in pos.items():
        res["case_" + k] = np.int32(v)
    unpacked = np.unpackbits(bits, axis=1)
    dt = {"port": np.int8, "pbits": np.uint8, "df": np.int8, "icao": np.int32, "has": np.int8, "cs": np.uint8,
          "csset": np.int8, "alt": np.int32, "altset": np.int8, "speed": np.uint64, "heading": np.uint64, "vrate": np.int32,
          "vrset": np.int8, "lat": np.uint64, "lon": np.uint64, "nmsgs": np.int32, "types": np.uint8}
    nan_bits = 0x7FF8000000000000
    for tag, filt, corr in G.CONFIGS:
        d = dups["cons" if corr == "Conservative" else "none"]
        pub = np.array([t for t in order if d[t] == -1], np.int64)
        dec = R.load_reference_decoder(filt, corr, "None")
        out = {k: [] for k in dt}
        G.run(dec, [(unpacked[t], float(ts[t]), 10.0) for t in pub], out, {})
        for k, v in out.items():
            if k == "types":
                continue
            a = np.array(v, dtype=dt[k])
            at_list = np.zeros((n,) + a.shape[1:], dtype=a.dtype)
            if k in ("speed", "heading", "lat", "lon"):
                at_list[:] = nan_bits
            if k == "pbits":
                at_list[:] = bits
            at_list[pub] = a                                           # the publication sequence -> list positions
            res["%s_%s" % (k, tag)] = at_list
        res["port_" + tag][d != -1] = 4
        res["df_" + tag][d != -1] = (bits[d != -1, 0] >> 3).astype(np.int8)
        res["icao_" + tag][d != -1] = -1
        res["pfix_" + tag] = res.pop("pbits_" + tag) ^ bits
        final = {k: [] for k in MG.KEYS}
        for key, p in dec.plane_dict.items():
            MG.put(final, int(key, 16) if key != "" else -1, p, p["last_seen"])
        for k in MG.KEYS:
            res["f_%s_%s" % (k, tag)] = np.array(final[k], dtype=MG.DT[k]).reshape((len(final[k]), 8) if k == "cs" else (len(final[k]),))
        nm, has, p = res["nmsgs_" + tag], res["has_" + tag], res["port_" + tag]
        if tag.startswith("all"):
            assert nm[pos["a0"]] == 1 and nm[pos["d1"]] == 2 and nm[pos["c_not"]] == 2 and nm[pos["c_q"]] == 1
            assert nm[pos["b_o0"]] == 2 and not np.isnan(res["lat_" + tag].view(np.float64)[pos["b_o0"]])
            assert nm[pos["g_again"]] == 2 and has[pos["h_q"]] == 0 and has[pos["h_known"]] == 1 and nm[pos["h_known"]] == 2
            assert nm[pos["fec_q"]] == 2          # A1's second message either way: the flipped hearing is a duplicate (Conservative) or fails parity
        print(tag, "published", len(pub), "of", n, "decoded", int((p == 1).sum()), "unknown", int((p == 2).sum()), "duplicates",
              int((p == 4).sum()), "planes", len(dec.plane_dict))
    path = os.path.join(ROOT, "tests", "golden", "g_dedup.npz")
    np.savez_compressed(path, **res)
    print(path, n, "pdus in 4 streams,", N_CALLS, "calls", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
