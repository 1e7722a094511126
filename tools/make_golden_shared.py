"""Record tests/golden/g_shared.npz: ONE UNMODIFIED reference decoder behind four receiver streams -- the fan-in of several
demod blocks into one decoder block (decoder.py:325-352) -- fed the streams' PDUs call by call, every call's PDUs in the
order ascending (timestamp, position in the call's list): the contract of ADSB_FLAG_STREAM_DECODE_SHARED
(include/adsb_hip.h SHARED DECODER), under the four (msg_filter, error_corr) configurations.  Container-only tool
(tools/ref_harness.py loads the reference by path); the tests read the .npz alone.

The decoder module's `time` is the PDU clock of tools/make_golden_decode.py (time() = the current PDU's timestamp).

Everything per PDU is stored at the PDU's LIST position: the calls concatenated, a call's list being its items in the order
they are passed, each item one stream's PDUs in stream order.
  fs, start[4]                          the streams' sample rate and start timestamps (stream 3's is negative)
  bits, stream, offset, call            the PDUs: 14 packed bytes, whose list, the record's sample offset, the call
  items_<c>                             call c's streams in the order its items are passed (a stream without PDUs: an empty item)
  ts                                    start[stream] + offset / fs, float64 -- the expression of the device code
  order                                 the publication order: list positions, calls in call order, (ts, position) inside
  port_<tag> ... nmsgs_<tag>, pfix_<tag>  per PDU what tests/golden/g_decode.npz holds (port, df, icao, the plane snapshot
                                        after the PDU, the repaired bits), so tests/test_decode.py's expected() reads them
  f_<k>_<tag>                           the final plane_dict, one entry per plane in its order: the fields of g_merge.npz
  case_b, case_c, case_d, case_e        list positions of the PDUs the cases below are about

The cases (tests/test_shared_decode.py asserts them from the file alone):
  (a) PA: even position frames only on stream 0, odd ones only on stream 2 -- it gets a position
  (b) an address/parity reply on stream 1 to AB, announced only on stream 3: earlier in time, later in the list -- known
  (c) an address/parity reply on stream 1 to AC, announced on stream 0 later in time but earlier in the list -- not known
  (d) a reply to AD on stream 1 and AD's announcement on stream 0 with bit-equal timestamps, items passed as [1, 0, 3]: the
      reply is published first -- not known
  (e) call 3, whose timestamps all precede call 2's: its reply to AE (announced in call 2) is known, calls publish in call order
  (f) stream 3 starts at -100 s: negative timestamps beside positive ones in one call"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decode_streams as S              # noqa: E402
import make_golden_decode as G          # noqa: E402
import make_golden_merge as MG          # noqa: E402
import ref_harness as R                 # noqa: E402

FS = 2e6
T0 = 1760000000.25
START = [T0, T0 + 0.5, T0 - 1.0, -100.0]
PA, AB, AC, AD, AE = 0x4B1A01, 0x3C65A2, 0xA0F003, 0x71BC04, 0x89ABCD
FLEET = [0x400000 + 4099 * k for k in range(10)] + [0, 0xFFFFFF]
N_CALLS = 5
ITEMS = [[0, 1, 2, 3], [1, 0, 3], [0, 1], [2, 3], [3, 2, 1, 0]]
# (call, [lo, hi) in seconds of the common clock -- stream 3: seconds after its own start) per stream
WINDOWS = [[(0, 0, 10), (1, 10, 20), (2, 20, 40), (4, 40, 60)],
           [(0, 0, 10), (1, 10, 20), (2, 20, 40), (4, 40, 60)],
           [(0, 0, 10), (3, 10, 20), (4, 20, 60)],
           [(0, 0, 10), (1, 10, 20), (3, 20, 40)]]


def call_of(stream, x):
    for c, lo, hi in WINDOWS[stream]:
        if lo <= x < hi:
            return c
    raise ValueError((stream, x))


def offset_of(stream, x):
    """The sample offset of the common clock's second x on `stream` (stream 3: x seconds after its start)."""
    rel = x if stream == 3 else x - (START[stream] - T0)
    off = int(round(rel * FS))
    assert abs(off - rel * FS) < 1e-3, (stream, x)
    return off


def lists(rng):
    """[(stream, x, packed bits, label)]"""
    ev = []

    def at(stream, x, b, label=""):
        b = np.asarray(b, np.uint8)
        ev.append((stream, x, np.packbits(b) if len(b) == 112 else b, label))
    for s in range(4):
        b, t = S.mixed(np.random.default_rng(900 + s), n=70, addresses=FLEET, t0=0.0, dt=(0.05, 1.2))
        span = 38.0 if s == 3 else 58.0
        x = np.round(t / t[-1] * span * 1e4) / 1e4 + 0.0501          # (a grid of 200 samples, off the round seconds below)
        for k in range(len(b)):
            at(s, float(x[k]), b[k])
    lat, lon = 47.1, 8.5
    # (a) even frames on stream 0, odd frames on stream 2
    at(0, 41.0, G.position(PA, 0, *G.cpr_encode(lat, lon, 0)), "a")
    at(2, 43.0, G.position(PA, 1, *G.cpr_encode(lat, lon, 1)), "a")
    at(0, 47.0, G.position(PA, 0, *G.cpr_encode(lat + 0.01, lon, 0)), "a")
    at(2, 49.0, G.position(PA, 1, *G.cpr_encode(lat + 0.01, lon, 1)), "a")
    # (b) announced on stream 3 only (second -95), the reply on stream 1
    at(3, 5.0, G.df11(AB, rng), "b_ann")
    at(1, 5.0, G.ap_fields(4, AB, rng, ac13=0x0B98), "b")
    # (c) the reply one second before the announcement, the announcement's item first
    at(0, 30.0, G.df11(AC, rng), "c_ann")
    at(1, 29.0, G.ap_fields(4, AC, rng, ac13=0x0B98), "c")
    # (d) bit-equal timestamps, the reply's item first
    at(1, 12.0, G.ap_fields(5, AD, rng), "d")
    at(0, 12.0, G.df11(AD, rng), "d_ann")
    # (e) announced in call 2 at second 35, the reply in call 3 at second 15
    at(0, 35.0, G.ident(AE, [5] * 8), "e_ann")
    at(2, 15.0, G.ap_fields(20, AE, rng, ac13=0x0B98), "e")
    # noise, and a reply with one wrong bit that "Conservative" repairs
    for s in range(4):
        at(s, 7.5, rng.integers(0, 2, 112).astype(np.uint8))
    at(2, 52.0, MG.flip(G.ident(PA, [9] * 8), 50))
    return ev


def main():
    rng = np.random.default_rng(20261201)
    ev = lists(rng)
    # the calls' lists
    rows = []
    for c in range(N_CALLS):
        for s in ITEMS[c]:
            mine = sorted((e for e in ev if e[0] == s and call_of(s, e[1]) == c), key=lambda e: e[1])
            rows += [(c, s, offset_of(s, x), b, label) for _, x, b, label in mine]
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
    pos = {label: k for k, r in enumerate(rows) for label in [r[4]] if label and label != "a"}
    assert ts[pos["d"]] == ts[pos["d_ann"]] and pos["d"] < pos["d_ann"]
    assert ts[pos["c"]] < ts[pos["c_ann"]] and pos["c_ann"] < pos["c"]
    assert ts[pos["b_ann"]] < 0 < ts[pos["b"]] and pos["b"] < pos["b_ann"]
    assert ts[call == 3].max() < ts[call == 2].min()
    res = {"fs": np.float64(FS), "start": start, "bits": bits, "stream": stream, "offset": offset, "call": call, "ts": ts,
           "order": order.astype(np.int32)}
    for c in range(N_CALLS):
        res["items_%d" % c] = np.array(ITEMS[c], np.int32)
    for k in "bcde":
        res["case_" + k] = np.array([pos[k + "_ann"], pos[k]], np.int32)
    unpacked = np.unpackbits(bits, axis=1)
    dt = {"port": np.int8, "pbits": np.uint8, "df": np.int8, "icao": np.int32, "has": np.int8, "cs": np.uint8,
          "csset": np.int8, "alt": np.int32, "altset": np.int8, "speed": np.uint64, "heading": np.uint64, "vrate": np.int32,
          "vrset": np.int8, "lat": np.uint64, "lon": np.uint64, "nmsgs": np.int32, "types": np.uint8}
    for tag, filt, corr in G.CONFIGS:
        dec = R.load_reference_decoder(filt, corr, "None")
        out = {k: [] for k in dt}
        G.run(dec, [(unpacked[t], float(ts[t]), 10.0) for t in order], out, {})
        for k, v in out.items():
            if k == "types":
                continue
            a = np.array(v, dtype=dt[k])
            at_list = np.zeros_like(a)
            at_list[order] = a                                         # publication order -> list positions
            res["%s_%s" % (k, tag)] = at_list
        res["pfix_" + tag] = res.pop("pbits_" + tag) ^ bits
        final = {k: [] for k in MG.KEYS}
        for key, p in dec.plane_dict.items():
            MG.put(final, int(key, 16) if key != "" else -1, p, p["last_seen"])
        for k in MG.KEYS:
            res["f_%s_%s" % (k, tag)] = np.array(final[k], dtype=MG.DT[k]).reshape((len(final[k]), 8) if k == "cs" else (len(final[k]),))
        p = res["port_" + tag]
        print(tag, "decoded", int((p == 1).sum()), "unknown", int((p == 2).sum()), "raised", int((p == 3).sum()), "planes",
              len(dec.plane_dict), "cases b c d e: port", [int(p[pos[k]]) for k in "bcde"], "has", [int(res["has_" + tag][pos[k]]) for k in "bcde"])
    path = os.path.join(ROOT, "tests", "golden", "g_shared.npz")
    np.savez_compressed(path, **res)
    print(path, n, "pdus in 4 streams,", N_CALLS, "calls", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
