"""Record tests/golden/g_expire.npz: the UNMODIFIED reference decoder with planes deleted from its plane_dict between PDUs --
`del self.plane_dict[key]` for every key with last_seen < cutoff, the sweep decoder.py:435-439 carries commented out, done
here by the tool at recorded points -- under the four (msg_filter, error_corr) configurations.  Container-only tool
(tools/ref_harness.py loads the reference by path); the tests read the .npz alone.

The decoder module's `time` is the PDU clock of tools/make_golden_decode.py (time() = the current PDU's timestamp), so
last_seen = int(timestamp).  The sequences are generated here: a handful of aircraft that appear, fall silent and return.

  bits, ts, snr, seq and, per configuration <tag>, port_ pfix_ df_ icao_ has_ cs_ csset_ alt_ altset_ speed_ heading_ vrate_
  vrset_ lat_ lon_ nmsgs_ types_                       one entry per PDU: tests/golden/g_decode.npz's layout
  del_seq, del_at, del_cutoff                          deletion point p: in sequence del_seq, in front of that sequence's PDU
                                                       number del_at (== the sequence's length: behind its last PDU), every
                                                       key with last_seen < del_cutoff is deleted
  del_removed_<tag>                                    the keys deleted at point p
  the plane_dict in front of every deletion point (b_*, b_pt_<tag> = p) and at the end of every sequence (f_*, f_seq_<tag>),
  one entry per plane in plane_dict's order: icao cs csset alt altset speed heading vrate vrset lat lon nmsgs as in
  tests/golden/g_planes.npz, and seen = last_seen
The reference's entry under the key "" (a repaired reply filed under no address) is no aircraft: it is left out of the sweep,
of the counts and of the recorded dicts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_decode as G          # noqa: E402
import make_golden_planes as P          # noqa: E402
import ref_harness as R                 # noqa: E402

A_, B_, C_, D_, E_, F_ = 0x4B1A01, 0x3C65A2, 0xA0F003, 0x000001, 0xFFFFFE, 0x71BC04


def flip(b, i):
    b = np.array(b, np.uint8)
    b[i] ^= 1
    return b


def life(T0, rng):
    """Five aircraft around four deletion points; every case of the issue's list but the clocks of the sequences below.
    T0's fraction is .25: T0 + x.9 falls in the whole second T0 + x + 1."""
    s, dels = [], []

    def at(t, b):
        s.append((b, T0 + t))
    lat, lon = 47.1, 8.5
    at(0.0, G.df11(A_, rng))
    at(0.4, G.ident(A_, [1, 2, 3, 4, 5, 6, 7, 8]))
    at(0.8, G.position(A_, 0, *G.cpr_encode(lat, lon, 0), alt12=0xC38))
    at(1.2, G.position(A_, 1, *G.cpr_encode(lat, lon, 1), alt12=0xC38))             # a fix
    at(1.6, G.velocity(A_, 1, 0, 300, 1, 120, 0, 9))
    at(2.0, G.ap_fields(4, A_, rng, ac13=0x0B98))                                   # known: an AC13 altitude
    at(3.0, G.df11(B_, rng))
    at(3.4, G.ident(B_, [2, 15, 2, 32, 48, 49, 50, 32]))
    at(3.8, G.ap_fields(20, B_, rng, ac13=0x1A98))
    at(4.0, G.ident(C_, [3] * 8, tc=2))                                             # C: extended squitters only
    at(4.5, G.position(C_, 0, *G.cpr_encode(-33.9, 151.2, 0), alt12=0x5B8))
    at(5.0, G.df11(E_, rng))
    at(5.4, G.ap_fields(0, E_, rng, ac13=0x0A18))
    at(6.0, rng.integers(0, 2, 112).astype(np.uint8))                               # noise
    at(6.4, G.ap_fields(4, F_, rng))                                                # an address nobody announced
    at(7.0, flip(G.ident(A_, [9] * 8), 50))                                         # one wrong bit: "Conservative" repairs it
    at(9.9, G.velocity(E_, 2, 1, 10, 0, 20, 1, 3))                                  # E: last_seen = int(T0) + 10
    at(10.4, G.df11(D_, rng))
    at(10.9, G.ident(D_, [4, 4, 4, 4, 32, 32, 32, 32]))                             # D: last_seen = int(T0) + 11
    # 1: A (last heard 7.0), B (3.8) and C (4.5) go; D and E stay
    dels.append((len(s), int(T0 + 7.0) + 1))
    at(12.0, G.position(C_, 1, *G.cpr_encode(-33.9, 151.2, 1), alt12=0x5B8))         # the even frame is gone: no fix
    at(12.4, G.ap_fields(4, A_, rng, ac13=0x0B98))                                  # unknown
    at(12.6, flip(G.ap_fields(4, A_, rng, ac13=0x0B98), 40))                        # ... and with one wrong bit
    at(12.8, G.ap_fields(5, B_, rng))                                               # unknown
    at(13.2, G.position(A_, 1, *G.cpr_encode(lat, lon, 1), alt12=0xC38))             # A again: num_msgs 1, no callsign, no fix
    at(13.6, G.ap_fields(4, A_, rng, ac13=0))                                       # known again (altitude stays the position's)
    at(14.0, G.position(A_, 0, *G.cpr_encode(lat, lon, 0), alt12=0xC38))             # a fix from the new pair
    at(14.4, G.df11(B_, rng))
    at(14.8, G.ap_fields(21, B_, rng))                                              # known again
    # 2: cutoff == D's last_seen: D stays, E (one second older) goes
    dels.append((len(s), int(T0) + 11))
    at(15.0, G.ap_fields(4, D_, rng, ac13=0x0C18))                                  # known
    at(15.2, G.ap_fields(4, E_, rng, ac13=0x0C18))                                  # unknown
    at(15.5, G.ident(E_, [5, 5, 5, 5, 5, 5, 5, 5]))                                 # E again: num_msgs 1
    at(15.8, G.velocity(A_, 1, 1, 5, 1, 7, 1, 2))                                   # A's row: a velocity, no callsign
    # 3: removes nothing
    dels.append((len(s), int(T0) - 5))
    at(16.0, G.ap_fields(16, E_, rng, ac13=0x0D98))
    at(16.4, G.ident(C_, [6] * 8))
    at(16.8, G.df11(A_, rng))
    # 4: a minute's time-out after two silent minutes: everybody goes (PLANE_TIMEOUT_S: now - last_seen > 60)
    dels.append((len(s), int(T0 + 140.0) - 60))
    at(140.0, G.ap_fields(4, A_, rng, ac13=0x0B98))
    at(140.3, G.ap_fields(4, D_, rng))
    at(140.6, G.ident(A_, [10] * 8))
    at(141.0, G.ap_fields(4, A_, rng, ac13=0x0B98))
    at(141.5, G.df11(D_, rng))
    at(290.0, G.position(D_, 0, *G.cpr_encode(1.0, 2.0, 0)))
    # 5: behind the last PDU: A (141.0) goes, D stays
    dels.append((len(s), int(T0 + 290.0) - 60))
    return s, dels


def truncation(rng):
    """Fractional and negative timestamps: int() truncates toward zero, so -0.5 is second 0 and -1.5 second -1."""
    s, dels = [], []
    s.append((G.df11(A_, rng), -100.75))
    s.append((G.ident(A_, [1] * 8), -99.5))
    s.append((G.df11(B_, rng), -1.5))                                               # last_seen -1
    s.append((G.df11(C_, rng), -0.5))                                               # last_seen 0 (floor would say -1)
    s.append((G.df11(D_, rng), 0.999))                                              # last_seen 0
    dels.append((len(s), -98))                                                      # A (-99) goes
    s.append((G.ap_fields(4, A_, rng), 1.25))                                       # unknown
    dels.append((len(s), 0))                                                        # B (-1) goes; C and D (0) stay
    for a in (B_, C_, D_):
        s.append((G.ap_fields(4, a, rng, ac13=0x0B98), 1.75))
    s.append((G.df11(B_, rng), 2.5))
    dels.append((len(s), 2))                                                        # the replies made C and D second 1: both go, B (2) stays
    for a in (B_, C_, D_):
        s.append((G.ap_fields(5, a, rng), 3.5))
    return s, dels


def far_clock(rng):
    """A clock beyond 2^31 (and 2^32): last_seen needs its 64 bits."""
    s, dels = [], []
    T = float(2 ** 31) + 1000.5
    s.append((G.df11(A_, rng), T))
    s.append((G.ident(B_, [7] * 8), T + 1))
    dels.append((len(s), 2 ** 31 + 1001))                                           # A goes, B (== cutoff) stays
    s.append((G.ap_fields(4, A_, rng), T + 2))
    s.append((G.ap_fields(4, B_, rng, ac13=0x0B98), T + 3))
    U = float(2 ** 33) + 0.5
    s.append((G.df11(A_, rng), U))
    s.append((G.df11(C_, rng), U + 70))
    dels.append((len(s), 2 ** 33 + 70 - 60))                                        # B (2^31 + 1003) and A (2^33) go
    for a in (A_, B_, C_):
        s.append((G.ap_fields(4, a, rng), U + 71))
    return s, dels


def backwards(rng):
    """Timestamps that go backwards: last_seen is the clock of the last PDU, not the largest clock."""
    s, dels = [], []
    s.append((G.df11(A_, rng), 1000.2))
    s.append((G.ident(A_, [1] * 8), 900.7))                                         # A: last_seen 900, largest 1000
    s.append((G.df11(B_, rng), 950.1))
    s.append((G.ident(B_, [2] * 8), 990.9))                                         # B: last_seen 990
    s.append((G.ident(C_, [3] * 8), 1200.0))
    s.append((G.ap_fields(4, C_, rng, ac13=0x0B98), 949.9))                         # C: last_seen 949 ("All Messages"), else 1200
    dels.append((len(s), 950))
    for a in (A_, B_, C_):
        s.append((G.ap_fields(4, a, rng, ac13=0x0C18), 1201.0))
    s.append((G.ident(A_, [4] * 8), 10.5))
    dels.append((len(s), 11))                                                       # A goes again
    return s, dels


def sequences(rng):
    return [life(1760000000.25, rng), truncation(rng), far_clock(rng), backwards(rng)]


SNAP = ("icao", "cs", "csset", "alt", "altset", "speed", "heading", "vrate", "vrset", "lat", "lon", "nmsgs", "seen")


def snapshot(dec, out, where):
    for icao, p in dec.plane_dict.items():
        if icao == "":
            continue
        out["where"].append(where)
        out["icao"].append(int(icao, 16))
        cs = p["callsign"]
        out["cs"].append(np.frombuffer((cs or "").encode().ljust(8, b"\0"), np.uint8))
        out["csset"].append(cs is not None)
        for name, flag, key in (("alt", "altset", "altitude"), ("vrate", "vrset", "vertical_rate")):
            out[flag].append(not P.isnan(p[key]))
            out[name].append(p[key] if out[flag][-1] else 0)
        for name, key in (("speed", "speed"), ("heading", "heading"), ("lat", "latitude"), ("lon", "longitude")):
            out[name].append(G.f64bits(p[key]))
        out["nmsgs"].append(p["num_msgs"])
        out["seen"].append(p["last_seen"])


def main():
    rng = np.random.default_rng(20261019)
    seqs = sequences(rng)
    rows = [(np.asarray(b, np.uint8), float(t)) for s, _ in seqs for b, t in s]
    snr = rng.uniform(0, 40, len(rows)).astype(np.float32)
    bits = np.array([b for b, _ in rows], dtype=np.uint8)
    res = {"bits": np.packbits(bits, axis=1), "ts": np.array([t for _, t in rows], np.float64), "snr": snr,
           "seq": np.array([i for i, (s, _) in enumerate(seqs) for _ in s], np.int32),
           "del_seq": np.array([i for i, (_, d) in enumerate(seqs) for _ in d], np.int32),
           "del_at": np.array([k for _, d in seqs for k, _ in d], np.int32),
           "del_cutoff": np.array([c for _, d in seqs for _, c in d], np.int64)}
    dt = {"port": np.int8, "pbits": np.uint8, "df": np.int8, "icao": np.int32, "has": np.int8, "cs": np.uint8, "csset": np.int8,
          "alt": np.int32, "altset": np.int8, "speed": np.uint64, "heading": np.uint64, "vrate": np.int32, "vrset": np.int8,
          "lat": np.uint64, "lon": np.uint64, "nmsgs": np.int32, "types": np.uint8, "seen": np.int64, "where": np.int32}
    for tag, filt, corr in G.CONFIGS:
        out = {k: [] for k in ("port", "pbits", "df", "icao", "has", "cs", "csset", "alt", "altset", "speed", "heading", "vrate",
                               "vrset", "lat", "lon", "nmsgs", "types")}
        before = {k: [] for k in SNAP + ("where",)}
        final = {k: [] for k in SNAP + ("where",)}
        removed, keys, k0, pt = [], {}, 0, 0
        for si, (s, dels) in enumerate(seqs):
            dec = R.load_reference_decoder(filt, corr, "None")
            for j in range(len(s) + 1):
                for at, cutoff in dels:
                    if at != j:
                        continue
                    snapshot(dec, before, pt)
                    gone = [k for k, p in dec.plane_dict.items() if k != "" and p["last_seen"] < cutoff]
                    for k in gone:
                        del dec.plane_dict[k]
                    removed.append(len(gone))
                    pt += 1
                if j < len(s):
                    b, t = s[j]
                    G.run(dec, [(np.asarray(b, np.uint8), float(t), float(snr[k0 + j]))], out, keys)
            snapshot(dec, final, si)
            k0 += len(s)
        for k, v in out.items():
            res["%s_%s" % (k, tag)] = np.array(v, dtype=dt[k])
        res["pfix_" + tag] = res.pop("pbits_" + tag) ^ res["bits"]
        res["del_removed_" + tag] = np.array(removed, np.int32)
        for pre, d, w in (("b", before, "pt"), ("f", final, "seq")):
            for k in SNAP:
                res["%s_%s_%s" % (pre, k, tag)] = np.array(d[k], dtype=dt[k]).reshape((len(d[k]), 8) if k == "cs" else (len(d[k]),))
            res["%s_%s_%s" % (pre, w, tag)] = np.array(d["where"], np.int32)
        p = res["port_" + tag]
        print(tag, "decoded", int((p == 1).sum()), "unknown", int((p == 2).sum()), "raised", int((p == 3).sum()), "removed", removed)
    path = os.path.join(ROOT, "tests", "golden", "g_expire.npz")
    np.savez_compressed(path, **res)
    print(path, len(bits), "pdus in", len(seqs), "sequences", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
