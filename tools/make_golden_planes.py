"""Record tests/golden/g_planes.npz: the UNMODIFIED reference decoder's final plane_dict, and the lines its print_planes
draws, for every sequence of tests/golden/g_decode.npz under the four (msg_filter, error_corr) configurations.  Container-only
tool (tools/ref_harness.py loads the reference by path); the tests read the .npz alone.

Per configuration <tag> (all_none, all_cons, es_none, es_cons), one entry per (sequence, plane) in the reference's own order
(sequence by sequence, inside a sequence plane_dict's insertion order):
  seq_<tag>      the sequence's number in g_decode.npz            icao_<tag>     the address; -1 for the key ""
  cs_<tag>       the callsign's bytes, NUL padded                 csset_<tag>    callsign is not None
  alt_<tag> / altset_<tag>, vrate_<tag> / vrset_<tag>             the integers, and whether the field is not NaN
  speed_<tag>, heading_<tag>, lat_<tag>, lon_<tag>                float64 bits
  nmsgs_<tag>    num_msgs                                         types_<tag>    Python type codes of the eight fields, as g_decode.npz
  line_<tag>     the string print_planes passes to screen.addstr for the plane, timestamp = the sequence's last PDU's
and keys: the entry's key order (cpr and last_seen included)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_decode as G          # noqa: E402
import ref_harness as R                 # noqa: E402

FIELDS = ("callsign", "altitude", "speed", "heading", "vertical_rate", "latitude", "longitude", "num_msgs")


class Screen:
    """curses' screen as print_planes uses it: addstr(row, col, text) recorded, refresh() ignored."""

    def __init__(self):
        self.lines = []

    def addstr(self, y, x, text, *attr):
        assert x == 0 and y == 2 + len(self.lines)
        self.lines.append(text)

    def refresh(self):
        pass


def isnan(v):
    return isinstance(v, float) and math.isnan(v)


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g_decode.npz"))
    bits = np.unpackbits(g["bits"], axis=1)
    ts, snr, seq = g["ts"], g["snr"], g["seq"]
    cut = np.concatenate([[0], np.flatnonzero(np.diff(seq)) + 1, [len(seq)]])
    res, keys = {}, None
    for tag, filt, corr in G.CONFIGS:
        out = {k: [] for k in ("seq", "icao", "cs", "csset", "alt", "altset", "speed", "heading", "vrate", "vrset", "lat", "lon",
                               "nmsgs", "types", "line")}
        for lo, hi in zip(cut[:-1], cut[1:]):
            dec = R.load_reference_decoder(filt, corr, "None")
            clock = G.Clock()
            dec.decode_packet.__func__.__globals__["time"] = clock
            for i in range(lo, hi):
                clock.now = float(ts[i])
                try:
                    dec.decode_packet(({"timestamp": float(ts[i]), "snr": float(snr[i])}, np.array(bits[i], dtype=np.uint8)))
                except Exception:
                    pass
            dec.screen = Screen()
            dec.timestamp = float(ts[hi - 1])
            dec.print_planes()
            assert len(dec.screen.lines) == len(dec.plane_dict)
            for (icao, p), line in zip(dec.plane_dict.items(), dec.screen.lines):
                keys = keys or tuple(p)
                assert tuple(p) == keys
                out["seq"].append(int(seq[lo]))
                out["icao"].append(int(icao, 16) if icao != "" else -1)      # "": a repaired reply filed under no address
                cs = p["callsign"]
                out["cs"].append(np.frombuffer((cs or "").encode().ljust(8, b"\0"), np.uint8))
                out["csset"].append(cs is not None)
                for name, flag, key in (("alt", "altset", "altitude"), ("vrate", "vrset", "vertical_rate")):
                    out[flag].append(not isnan(p[key]))
                    out[name].append(p[key] if out[flag][-1] else 0)
                for name, key in (("speed", "speed"), ("heading", "heading"), ("lat", "latitude"), ("lon", "longitude")):
                    out[name].append(G.f64bits(p[key]))
                out["nmsgs"].append(p["num_msgs"])
                out["types"].append([G.tcode(p[k]) for k in FIELDS])
                out["line"].append(line)
        dt = {"seq": np.int32, "icao": np.int32, "cs": np.uint8, "csset": np.int8, "alt": np.int32, "altset": np.int8,
              "speed": np.uint64, "heading": np.uint64, "vrate": np.int32, "vrset": np.int8, "lat": np.uint64, "lon": np.uint64,
              "nmsgs": np.int32, "types": np.uint8, "line": np.str_}
        for k, v in out.items():
            res["%s_%s" % (k, tag)] = np.array(v, dtype=dt[k])
        print(tag, len(out["icao"]), "planes")
    res["keys"] = np.array(keys)
    path = os.path.join(ROOT, "tests", "golden", "g_planes.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
