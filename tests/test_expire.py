"""Plane ages on the CPU (ADSB_FLAG_PLANE_AGES: last_seen on the device, adsb_planes_seen / adsb_stream_planes_seen,
adsb_planes_expire / adsb_stream_planes_expire): the emulated kernels (tests/sim/expire_driver.cpp over the decoders of
decode_driver.cpp and fleet_driver.cpp) against tests/golden/g_expire.npz -- the UNMODIFIED reference decoder with
`del plane_dict[key]` applied between PDUs at recorded points -- and against a plain-Python model (decode_replay.Decoder with
last_seen and the sweep), itself checked against the golden first; the host functions _native.plane_entry(last_seen=) and
blocks.decoder(plane_timeout=); the declared symbols and the kernels' resources.

What a green run here does NOT cover: the driver restates the host's argument rules, launch order and bookkeeping
(adsb_hip.hip adsb_planes_expire / adsb_stream_planes_expire / fleet_rehash); the host code itself runs in
tests/test_gpu_expire.py only."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
import test_decode as TD
import test_planes as TP
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
EXPIRE_SO = os.path.join(SIM_DIR, "libadsb_expire_sim.so")
GOLD = os.path.join(HERE, "golden", "g_expire.npz")
CONFIGS = TD.CONFIGS
CHUNK, TOP = TP.CHUNK, TP.TOP
INT64_MIN = -(1 << 63)
GARBAGE = 0x5A5A5A5A5A5A5A5A          # what a last_seen entry holds before its plane's first fold: never read
vp = ctypes.c_void_p


def expire_lib():
    srcs = [os.path.join(SIM_DIR, f) for f in ("expire_driver.cpp", "planes_driver.cpp", "fleet_driver.cpp", "decode_driver.cpp", "sim_support.h",
                                               "hipsim.h")] + \
        [os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not (os.path.exists(EXPIRE_SO) and all(os.path.getmtime(EXPIRE_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", EXPIRE_SO])
    lib = ctypes.CDLL(EXPIRE_SO)
    lib.sim_exp_fleet_open.restype = ctypes.c_void_p
    lib.sim_exp_fleet_slot_of.restype = ctypes.c_longlong
    lib.sim_exp_fleet_home.restype = ctypes.c_uint
    lib.sim_fleet_taken.restype = ctypes.c_longlong
    lib.sim_fleet_gen_max.restype = ctypes.c_uint
    lib.sim_fleet_get_call.restype = ctypes.c_ulonglong
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = expire_lib()
    assert lib.sim_planes_chunk() == CHUNK
    assert lib.sim_dec_row_bytes() == N.DECODED_DTYPE.itemsize and lib.sim_dec_plane_bytes() == 88 and lib.sim_fleet_slot_bytes() == 104
    return lib


@pytest.fixture(scope="module")
def ge():
    return np.load(GOLD)


# ---- the model: decode_replay's decoder with last_seen and the sweep -----------------------------------------------------------
class Model:
    """decode_replay.Decoder plus plane_dict's last_seen (it moves where num_msgs moves) and `del plane_dict[key]`."""

    def __init__(self, filt, corr):
        self.d = D.Decoder(filt, corr)
        self.seen = {}

    def row(self, b, t):
        before = {a: p["n"] for a, p in self.d.planes.items()}
        r = self.d.row(b, t)
        for a, p in self.d.planes.items():
            if before.get(a) != p["n"]:
                self.seen[a] = int(t)
        return r

    def rows(self, bs, ts):
        return S.to_rows([self.row(b, t) for b, t in zip(bs, ts)])

    def sweep(self, cutoff):
        gone = [a for a in self.d.planes if self.seen[a] < cutoff]
        for a in gone:
            del self.d.planes[a], self.seen[a]
        return len(gone)

    def snapshot(self):
        return TP.plane_rows(self.d.planes), np.array([self.seen[a] for a in sorted(self.d.planes)], np.int64)


# ---- the golden's shape --------------------------------------------------------------------------------------------------------
def sequences(ge):
    """[(slice of the sequence's PDUs, [(point number, PDU number inside the sequence, cutoff)])]"""
    out = []
    for seq, sl in enumerate(TD.seq_slices(ge["seq"])):
        pts = [(int(p), int(ge["del_at"][p]), int(ge["del_cutoff"][p])) for p in np.flatnonzero(ge["del_seq"] == seq)]
        out.append((sl, pts))
    return out


def gold_dict(ge, tag, pre, where):
    """The recorded plane_dict `pre` ("b": in front of deletion point `where`, "f": at the end of sequence `where`), ascending
    address: TP.check_against_golden's dict and the last_seen array."""
    w = ge["%s_%s_%s" % (pre, "pt" if pre == "b" else "seq", tag)]
    m = np.flatnonzero(w == where)
    m = m[np.argsort(ge["%s_icao_%s" % (pre, tag)][m], kind="stable")]
    e = {k: ge["%s_%s_%s" % (pre, k, tag)][m] for k in ("icao", "cs", "csset", "alt", "altset", "speed", "heading", "vrate", "vrset",
                                                       "lat", "lon", "nmsgs")}
    return e, ge["%s_seen_%s" % (pre, tag)][m]


def segments(n, pts, extra=()):
    """The calls of a sequence of n PDUs: [(lo, hi, the deletion points in front of PDU lo)] and the points behind the last
    PDU; no call spans a deletion point; extra: more cuts."""
    cuts = sorted({0, n} | {at for _, at, _ in pts} | {int(c) for c in extra if 0 < c < n})
    segs = [(lo, hi, [p for p in pts if p[1] == lo]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    if not segs:
        segs = [(0, 0, [p for p in pts if p[1] == 0])]
    return segs, [p for p in pts if p[1] == n and n > 0]


CHUNKINGS = ("points", "single", "random")


def extra_cuts(how, n, rng):
    return {"points": (), "single": range(n), "random": rng.integers(1, max(n, 2), 6)}[how]


def run_golden(ge, tag, make, how):
    """Every sequence of the golden through a decoder of its own (make() -> an object with call(bits, ts), expire(cutoff) ->
    removed, snapshot() -> (rows, seen)): rows, the plane_dict in front of every deletion point and at the end with
    last_seen, and the numbers removed."""
    rng = np.random.default_rng(5)
    n_pts = 0
    for seq, (sl, pts) in enumerate(sequences(ge)):
        dec = make()
        bits, ts = ge["bits"][sl], ge["ts"][sl]
        got = np.zeros(len(bits), dtype=N.DECODED_DTYPE)
        segs, tail = segments(len(bits), pts, extra_cuts(how, len(bits), rng))

        def sweep(points):
            nonlocal n_pts
            for p, _, cutoff in points:
                rows, seen = dec.snapshot()
                e, eseen = gold_dict(ge, tag, "b", p)
                TP.check_against_golden(rows, e, (tag, "point", p))
                assert np.array_equal(seen, eseen), (tag, p, seen, eseen)
                assert dec.expire(cutoff) == int(ge["del_removed_" + tag][p]), (tag, p)
                n_pts += 1
        for lo, hi, points in segs:
            sweep(points)
            if hi > lo:
                got[lo:hi] = dec.call(bits[lo:hi], ts[lo:hi])
        sweep(tail)
        TD.check_rows(got, ge, tag, sl)
        rows, seen = dec.snapshot()
        e, eseen = gold_dict(ge, tag, "f", seq)
        TP.check_against_golden(rows, e, (tag, "end", seq))
        assert np.array_equal(seen, eseen), (tag, seq)
        if hasattr(dec, "close"):
            dec.close()
    assert n_pts == len(ge["del_at"])


def test_golden_holds_the_cases(ge):
    """What tools/make_golden_expire.py promises, read from the file alone."""
    assert len(TD.seq_slices(ge["seq"])) == 4 and len(ge["del_at"]) == 12
    a = ge["del_removed_all_none"]
    assert (a == 0).any() and (a >= 3).any() and a.sum() >= 15
    ts, cut = ge["ts"], ge["del_cutoff"]
    assert (ts < 0).any() and (ts != np.floor(ts)).any() and ts.max() > 2.0 ** 33 and cut.max() > 2 ** 33 and cut.min() < 0
    back = TD.seq_slices(ge["seq"])[3]
    assert (np.diff(ts[back]) < 0).any()
    # an address/parity reply known, unknown after the expiry, known after the aircraft is heard again
    sl = TD.seq_slices(ge["seq"])[0]
    icao, port, has = ge["icao_all_none"][sl], ge["port_all_none"][sl], ge["has_all_none"][sl]
    df = ge["df_all_none"][sl]
    ap = np.flatnonzero((icao == 0x4B1A01) & np.isin(df, (0, 4, 5, 16, 20, 21)))
    assert has[ap].tolist() == [1, 0, 1, 0, 1]                  # (the reply with a wrong bit is filed under another address)
    # a plane that returns starts over: num_msgs 1, no callsign
    k = int(np.flatnonzero((icao == 0x4B1A01) & (df == 17) & (has == 1))[4])
    assert ge["nmsgs_all_none"][sl][k] == 1 and ge["csset_all_none"][sl][k] == 0 and port[k] == 0
    # cutoff == last_seen stays, cutoff - 1 goes
    e, seen = gold_dict(ge, "all_none", "b", 1)
    c = int(ge["del_cutoff"][1])
    assert (seen == c).any() and (seen == c - 1).any() and ge["del_removed_all_none"][1] == int((seen < c).sum()) == 1


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_model_equals_golden(ge, tag, filt, corr):
    class Dec(Model):
        def __init__(self):
            Model.__init__(self, filt, corr)
        call = Model.rows
        expire = Model.sweep
    run_golden(ge, tag, Dec, "points")


# ---- one decoder on the emulated kernels ---------------------------------------------------------------------------------------
class AgedDecoder(TD.SimDecoder):
    """test_decode.SimDecoder with the last_seen array beside its planes; seen=False: the array is not passed (no flag)."""

    def __init__(self, lib, filt, corr, seen=True):
        TD.SimDecoder.__init__(self, lib, filt, corr)
        self.seen = np.full(1 << 24, GARBAGE, dtype=np.int64) if seen else None
        self.touched = set()

    def call(self, bits14, ts, grid=4):
        b = np.ascontiguousarray(bits14, dtype=np.uint8).copy()
        t = np.ascontiguousarray(ts, dtype=np.float64)
        rows = np.zeros(len(b), dtype=N.DECODED_DTYPE)
        rc = self.lib.sim_exp_dec_pdus(b.ctypes.data_as(vp), t.ctypes.data_as(vp), ctypes.c_int(len(b)), ctypes.c_int(grid),
                                       self.table.ctypes.data_as(vp), self.st.ctypes.data_as(vp), self.planes.ctypes.data_as(vp),
                                       self.seen.ctypes.data_as(vp) if self.seen is not None else None,
                                       ctypes.c_uint(self.epoch), ctypes.c_ulonglong(self.next), ctypes.c_int(self.fec), ctypes.c_int(self.all),
                                       rows.ctypes.data_as(vp))
        assert rc == 0, rc
        self.next += 1
        self.touched |= {int(a) for a in rows["icao"] if a >= 0}
        return rows

    def expire(self, cutoff, ranges=None, grid=2):
        """adsb_planes_expire over the chunks of every address a row has named (ranges None), or over [(lo, hi)]."""
        total = 0
        for lo, hi in (TP.windows(self.touched) if ranges is None else ranges):
            n = ctypes.c_longlong(-1)
            rc = self.lib.sim_exp_dense_expire(self.table.ctypes.data_as(vp), self.planes.ctypes.data_as(vp), self.seen.ctypes.data_as(vp),
                                               ctypes.c_uint(self.epoch), ctypes.c_uint(lo), ctypes.c_uint(hi), ctypes.c_int(grid),
                                               ctypes.c_longlong(cutoff), ctypes.byref(n))
            assert rc == 0, rc
            total += n.value
        return total

    def snapshot(self, ranges=None, grid=2, rows=True, seen=True):
        cap = len(self.touched) + 8
        rs, ss = [], []
        for lo, hi in (TP.windows(self.touched) if ranges is None else ranges):
            r = np.zeros(cap, dtype=N.DECODED_DTYPE)
            s = np.zeros(cap, dtype=np.int64)
            n = ctypes.c_int(-1)
            rc = self.lib.sim_exp_dense_seen(self.table.ctypes.data_as(vp), self.planes.ctypes.data_as(vp), self.seen.ctypes.data_as(vp),
                                             ctypes.c_uint(self.epoch), ctypes.c_uint(lo), ctypes.c_uint(hi), ctypes.c_int(grid),
                                             ctypes.c_int(cap), r.ctypes.data_as(vp) if rows else None,
                                             s.ctypes.data_as(vp) if seen else None, ctypes.byref(n))
            assert rc == 0, rc
            rs.append(r[:n.value])
            ss.append(s[:n.value])
        return np.concatenate(rs), np.concatenate(ss)

    def plain_snapshot(self):
        return TP.dense_over(self.lib, self, sorted(self.touched))


@pytest.mark.parametrize("how", CHUNKINGS)
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_dense_equals_golden(sim, ge, tag, filt, corr, how):
    """The golden through the decode step with a last_seen array, k_ages_expire at the recorded points and k_ages_emit in front
    of each: rows, plane_dict with last_seen and the numbers removed, under three chunkings of the PDUs into calls."""
    shared = AgedDecoder(sim, filt, corr)

    def make():
        shared.reset()
        shared.touched = set()
        return shared
    run_golden(ge, tag, make, how)


def ident(aa, rng):
    return TP.ident(aa, rng)


def df11(aa):
    f = np.zeros(112, np.uint8)
    f[:5], f[5:8], f[8:32] = S.ib(11, 5), S.ib(5, 3), S.ib(aa, 24)
    f[32:56] = S.ib(S.M.crc24(f[:32]), 24)
    return np.packbits(f)


def snap_es(aa, tc=28):
    """An extended squitter the decoder accepts without touching the plane (TC 0, 5-8, 20-31: kEvSnap)."""
    return np.packbits(S.es(aa, tc, np.zeros(51, np.uint8)))


def ap4(aa, rng):
    return np.packbits(S.ap(4, aa, rng))


def check_dense(dec, model, what=""):
    rows, seen = dec.snapshot()
    erows, eseen = model.snapshot()
    TP.rows_equal(rows, erows)
    assert np.array_equal(seen, eseen), what
    TP.rows_equal(dec.plain_snapshot(), erows)                 # the plain snapshot (k_planes_emit) agrees


def test_dense_scan_edges(sim):
    """Planes at addresses 0, 1, 2047, 2048, 0xFFFFFE, 0xFFFFFF; the even / odd pair of one 16-byte load with one stale and one
    fresh, both ways round; a chunk whose planes are all stale; an announced address without a plane (left alone); every
    survivor and every expired address answered by an address/parity reply afterwards."""
    rng = np.random.default_rng(61)
    edge = [0, 1, CHUNK - 1, CHUNK, 0xFFFFFE, 0xFFFFFF]
    pairs = [0x300010, 0x300011, 0x300020, 0x300021]            # stale/fresh and fresh/stale
    full = list(range(5 * CHUNK, 5 * CHUNK + 40))               # every plane of this chunk goes
    dec, mod = AgedDecoder(sim, "All Messages", "None"), Model("All Messages", "None")
    t0 = 5000.5
    old = edge[::2] + [pairs[0], pairs[3]] + full
    new = edge[1::2] + [pairs[1], pairs[2]]
    b = [ident(a, rng) for a in old] + [ident(a, rng) for a in new]
    t = [t0 + 0.01 * k for k in range(len(old))] + [t0 + 100 + 0.01 * k for k in range(len(new))]
    TP.rows_equal(dec.call(b, t), mod.rows(b, t))
    check_dense(dec, mod)
    cutoff = int(t0) + 50
    for grid in (3,):
        assert dec.expire(cutoff, grid=grid) == mod.sweep(cutoff) == len(old)
    check_dense(dec, mod)
    assert dec.snapshot(ranges=[(5 * CHUNK, 6 * CHUNK)])[0].size == 0
    assert (dec.table[old] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (dec.table[new] != np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert dec.expire(cutoff) == 0                                                    # nothing left below it
    b = [ap4(a, rng) for a in old + new]
    t = [t0 + 200 + 0.01 * k for k in range(len(b))]
    got = dec.call(b, t)
    TP.rows_equal(got, mod.rows(b, t))
    assert not (got["present"][:len(old)] & N.DEC_HAS_PLANE).any() and (got["present"][len(old):] & N.DEC_HAS_PLANE).all()
    b = [ident(a, rng) for a in old[:5]] + [ap4(a, rng) for a in old[:5]]              # heard again: fresh entries
    t = [t0 + 300 + 0.01 * k for k in range(len(b))]
    got = dec.call(b, t)
    TP.rows_equal(got, mod.rows(b, t))
    assert got["num_msgs"].tolist() == [1] * 5 + [2] * 5
    check_dense(dec, mod)
    # announced, no plane: under "Extended Squitter Only" a DF 11 reply announces its address and reaches no update_plane
    es_dec = AgedDecoder(sim, "Extended Squitter Only", "None")
    got = es_dec.call([df11(0x123456), ident(0x123457, rng)], [10.5, 11.5])
    assert (got["present"] & N.DEC_HAS_PLANE).tolist() == [0, 1]
    key = es_dec.table[0x123456]
    assert key != np.uint64(0xFFFFFFFFFFFFFFFF) and es_dec.seen[0x123456] == GARBAGE
    assert es_dec.expire(1 << 62) == 1
    assert es_dec.table[0x123456] == key and es_dec.table[0x123457] == np.uint64(0xFFFFFFFFFFFFFFFF)


def test_dense_whole_address_space_in_one_scan(sim):
    """One k_ages_expire over 0 .. 2^24 by a grid that does not divide the chunks, among untouched garbage last_seen entries."""
    rng = np.random.default_rng(62)
    addr = TP.EDGE + [0x400000 + 523 * k for k in range(120)]
    dec, mod = AgedDecoder(sim, "All Messages", "Conservative"), Model("All Messages", "Conservative")
    b, t = S.mixed(rng, n=900, addresses=addr, t0=1760000000.5)
    TP.rows_equal(dec.call(b, t), mod.rows(b, t))
    cutoff = int(np.median(list(mod.seen.values())))
    n = mod.sweep(cutoff)
    assert 20 < n < len(addr) - 20
    assert dec.expire(cutoff, ranges=[(0, TOP)], grid=5) == n
    check_dense(dec, mod)
    b, t = S.mixed(rng, n=500, addresses=addr, t0=float(t[-1]) + 1)
    TP.rows_equal(dec.call(b, t), mod.rows(b, t))
    check_dense(dec, mod)


def test_last_seen_moves_iff_num_msgs_moves(sim):
    """A segment whose last record is a kEvSnap record keeps the clock of the last record that reached update_plane; a call
    with nothing but such records writes no last_seen at all."""
    rng = np.random.default_rng(63)
    a = 0x0ABCDE
    dec, mod = AgedDecoder(sim, "All Messages", "None"), Model("All Messages", "None")
    b, t = [ident(a, rng), snap_es(a, 28), snap_es(a, 0)], [100.5, 200.5, 300.5]
    got = dec.call(b, t)
    TP.rows_equal(got, mod.rows(b, t))
    assert got["num_msgs"].tolist() == [1, 1, 1] and got["port"].tolist() == [N.DEC_DECODED, N.DEC_UNKNOWN, N.DEC_NONE]
    assert dec.snapshot()[1].tolist() == [100] == mod.snapshot()[1].tolist()
    TP.rows_equal(dec.call([snap_es(a, 6)], [400.5]), mod.rows([snap_es(a, 6)], [400.5]))
    assert dec.snapshot()[1].tolist() == [100]
    b, t = [ap4(a, rng), snap_es(a, 28), ap4(a, rng), snap_es(a, 7)], [500.9, 600.5, 450.2, 700.5]
    got = dec.call(b, t)
    TP.rows_equal(got, mod.rows(b, t))
    assert got["num_msgs"].tolist() == [2, 2, 3, 3] and dec.snapshot()[1].tolist() == [450]      # the last event, not the largest


def test_no_op_expiry_changes_no_byte(sim):
    """A cutoff of INT64_MIN removes nothing; the rows decoded after it and the snapshots around it are those of a run without."""
    rng = np.random.default_rng(64)
    addr = [0x10, 0x11, 0x7FF, 0x800, 0xABCDEF] + [0x500000 + 97 * k for k in range(40)]
    b, t = S.mixed(rng, n=700, addresses=addr)
    with_, without = AgedDecoder(sim, "All Messages", "Conservative"), AgedDecoder(sim, "All Messages", "Conservative")
    r0, r1 = with_.call(b[:400], t[:400]), without.call(b[:400], t[:400])
    before = with_.snapshot()
    table, planes = with_.table.copy(), with_.planes[:0x900 * 88].copy()
    assert with_.expire(INT64_MIN, ranges=[(0, TOP)], grid=4) == 0
    assert np.array_equal(table, with_.table) and np.array_equal(planes, with_.planes[:0x900 * 88])
    after = with_.snapshot()
    TP.rows_equal(before[0], after[0])
    assert np.array_equal(before[1], after[1])
    S.assert_rows_equal(with_.call(b[400:], t[400:]), without.call(b[400:], t[400:]))
    S.assert_rows_equal(r0, r1)
    a, c = with_.snapshot(), without.snapshot()
    TP.rows_equal(a[0], c[0])
    assert np.array_equal(a[1], c[1])
    # rows alone, last_seen alone
    TP.rows_equal(with_.snapshot(seen=False)[0], a[0])
    assert np.array_equal(with_.snapshot(rows=False)[1], a[1])


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_without_the_array_the_decode_step_writes_the_parents_bytes(sim, ge, tag, filt, corr):
    """DecArgs::seen null (no flag): the rows, the table and the planes are those of decode_driver.cpp's sim_dec_pdus, which
    knows no last_seen."""
    g = np.load(TD.GOLD)
    sl = TD.seq_slices(g["seq"])[-1]                      # the long mixed sequence
    a, b = AgedDecoder(sim, filt, corr, seen=False), TD.SimDecoder(sim, filt, corr)
    for lo in range(sl.start, sl.stop, 300):
        hi = min(lo + 300, sl.stop)
        S.assert_rows_equal(a.call(g["bits"][lo:hi], g["ts"][lo:hi]), b.call(g["bits"][lo:hi], g["ts"][lo:hi]))
    touched = sorted(a.touched)
    assert np.array_equal(a.table[touched], b.table[touched])
    pa, pb = a.planes.reshape(-1, 88), b.planes.reshape(-1, 88)
    assert np.array_equal(pa[touched], pb[touched])


# ---- the fleet on the emulated kernels -----------------------------------------------------------------------------------------
class AgedFleet:
    """The decoders of n streams with last_seen beside the store's slots (expire_driver.cpp's handle)."""

    def __init__(self, lib, n_streams, filt, corr, slots=256):
        self.lib, self.n = lib, n_streams
        self.h = vp(lib.sim_exp_fleet_open(ctypes.c_int(n_streams), ctypes.c_longlong(slots), ctypes.c_int(corr == "Conservative"),
                                           ctypes.c_int(filt == "All Messages")))

    def close(self):
        self.lib.sim_exp_fleet_close(self.h)

    def call(self, bits14, ts, stream, grid=3):
        b = np.ascontiguousarray(bits14, dtype=np.uint8)
        t = np.ascontiguousarray(ts, dtype=np.float64)
        s = np.ascontiguousarray(stream, dtype=np.int32)
        rows = np.zeros(len(b), dtype=N.DECODED_DTYPE)
        rc = self.lib.sim_exp_fleet_call(self.h, b.ctypes.data_as(vp), t.ctypes.data_as(vp), s.ctypes.data_as(vp), ctypes.c_int(len(b)),
                                         ctypes.c_int(grid), rows.ctypes.data_as(vp))
        assert rc == 0, rc
        return rows

    def expire(self, cutoffs, streams=None, grid=2):
        cut = np.ascontiguousarray(cutoffs, dtype=np.int64)
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        n = ctypes.c_longlong(-1)
        rc = self.lib.sim_exp_fleet_expire(self.h, None if sel is None else sel.ctypes.data_as(vp), ctypes.c_int(0 if sel is None else len(sel)),
                                           cut.ctypes.data_as(vp), ctypes.c_int(grid), ctypes.byref(n))
        assert rc == 0, rc
        return n.value

    def snapshot(self, streams=None, grid=2, rows=True, seen=True):
        cap = self.stats()["planes"]
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        k = self.n if sel is None else len(sel)
        r, s = np.zeros(cap, dtype=N.DECODED_DTYPE), np.zeros(cap, dtype=np.int64)
        first = np.zeros(k + 1, dtype=np.int32)
        n = ctypes.c_int(-1)
        rc = self.lib.sim_exp_fleet_seen(self.h, None if sel is None else sel.ctypes.data_as(vp), ctypes.c_int(k), ctypes.c_int(grid),
                                         ctypes.c_int(cap), r.ctypes.data_as(vp) if rows else None, s.ctypes.data_as(vp) if seen else None,
                                         first.ctypes.data_as(vp), ctypes.byref(n))
        assert rc == 0, rc
        return r[:n.value], s[:n.value], first

    def plain_snapshot(self):
        cap = self.stats()["planes"]
        r = np.zeros(cap, dtype=N.DECODED_DTYPE)
        first = np.zeros(self.n + 1, dtype=np.int32)
        n = ctypes.c_int(-1)
        rc = self.lib.sim_planes_fleet(self.h, None, ctypes.c_int(0), ctypes.c_int(2), ctypes.c_int(cap), r.ctypes.data_as(vp),
                                       first.ctypes.data_as(vp), ctypes.byref(n))
        assert rc == 0, rc
        return r[:n.value], first

    def reset(self, stream):
        assert self.lib.sim_exp_fleet_reset(self.h, ctypes.c_int(stream)) == 0

    def stats(self):
        v = [ctypes.c_longlong() for _ in range(4)]
        self.lib.sim_fleet_stats(self.h, *[ctypes.byref(x) for x in v])
        return dict(planes=v[0].value, capacity=v[1].value, grows=v[2].value, used=v[3].value)

    def taken(self):
        return int(self.lib.sim_fleet_taken(self.h))

    def slot_of(self, stream, addr):
        return int(self.lib.sim_exp_fleet_slot_of(self.h, ctypes.c_int(stream), ctypes.c_uint(addr)))

    def home(self, stream, addr, cap):
        return int(self.lib.sim_exp_fleet_home(self.h, ctypes.c_int(stream), ctypes.c_uint(addr), ctypes.c_longlong(cap)))


@pytest.mark.parametrize("how", CHUNKINGS[:2])
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_fleet_one_stream_per_sequence_equals_golden(sim, ge, tag, filt, corr, how):
    class Dec(AgedFleet):
        def __init__(self):
            AgedFleet.__init__(self, sim, 1, filt, corr)

        def call(self, b, t):
            return AgedFleet.call(self, b, t, np.zeros(len(b), np.int32))

        def expire(self, cutoff):
            return AgedFleet.expire(self, [cutoff])

        def snapshot(self):
            return AgedFleet.snapshot(self)[:2]
    run_golden(ge, tag, Dec, how)


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_fleet_sequences_as_streams_of_one_store_equal_golden(sim, ge, tag, filt, corr):
    """The golden's four sequences as streams 0 .. 3 of ONE 256-slot store, round by round: every stream's next call, its
    deletion points in front (adsb_stream_planes_expire with that stream selected and its own cutoff: the others lose
    nothing).  Rows, the plane_dict with last_seen at every point and at the end, the numbers removed, the planes counter."""
    seqs = sequences(ge)
    f = AgedFleet(sim, len(seqs), filt, corr)
    plans = [segments(sl.stop - sl.start, pts, (3, 7)) for sl, pts in seqs]
    got = np.zeros(len(ge["bits"]), dtype=N.DECODED_DTYPE)
    live = [0] * len(seqs)

    def sweep(s, points):
        for p, _, cutoff in points:
            rows, seen, first = f.snapshot([s])
            e, eseen = gold_dict(ge, tag, "b", p)
            TP.check_against_golden(rows, e, (tag, p))
            assert np.array_equal(seen, eseen) and first.tolist() == [0, len(rows)]
            n = f.expire([cutoff], [s])
            assert n == int(ge["del_removed_" + tag][p])
            live[s] = len(rows) - n
            others = f.snapshot()[2]
            assert f.stats()["planes"] == others[-1]
    for rnd in range(max(len(p[0]) for p in plans)):
        bs, ts, ss, where = [], [], [], []
        for s, ((segs, _), (sl, _)) in enumerate(zip(plans, seqs)):
            if rnd >= len(segs):
                continue
            lo, hi, points = segs[rnd]
            sweep(s, points)
            idx = np.arange(sl.start + lo, sl.start + hi)
            bs.append(ge["bits"][idx]); ts.append(ge["ts"][idx]); ss.append(np.full(len(idx), s, np.int32)); where.append(idx)
        if bs and sum(len(x) for x in bs):
            got[np.concatenate(where)] = f.call(np.concatenate(bs), np.concatenate(ts), np.concatenate(ss))
    for s, (_, tail) in enumerate(plans):
        sweep(s, tail)
    TD.check_rows(got, ge, tag)
    rows, seen, first = f.snapshot()
    for s in range(len(seqs)):
        e, eseen = gold_dict(ge, tag, "f", s)
        TP.check_against_golden(rows[first[s]:first[s + 1]], e, (tag, "end", s))
        assert np.array_equal(seen[first[s]:first[s + 1]], eseen)
    TP.rows_equal(f.plain_snapshot()[0], rows)
    assert f.stats()["planes"] == len(rows) and f.stats()["capacity"] == 256
    f.close()


class FleetModel:
    def __init__(self, n, filt="All Messages", corr="None"):
        self.cfg = (filt, corr)
        self.m = [Model(filt, corr) for _ in range(n)]

    def call(self, b, t, s):
        return S.to_rows([self.m[int(k)].row(x, y) for x, y, k in zip(b, t, s)])

    def reset(self, s):
        self.m[s] = Model(*self.cfg)

    def planes(self):
        return sum(len(m.d.planes) for m in self.m)


def check_fleet(f, mod, what=""):
    rows, seen, first = f.snapshot()
    for s, m in enumerate(mod.m):
        erows, eseen = m.snapshot()
        TP.rows_equal(rows[first[s]:first[s + 1]], erows)
        assert np.array_equal(seen[first[s]:first[s + 1]], eseen), (what, s)
    assert f.stats()["planes"] == mod.planes() == len(rows)
    TP.rows_equal(f.plain_snapshot()[0], rows)


def probe_all(f, mod, addrs, t, rng):
    """An address/parity reply to every (stream, address): known exactly where the model still has the plane."""
    b = [ap4(a, rng) for s, a in addrs]
    ss = [s for s, a in addrs]
    ts = [t + 0.001 * k for k in range(len(b))]
    got = f.call(b, ts, ss)
    S.assert_rows_equal(got, mod.call(b, ts, ss))
    return got


def cluster_addresses(f, n, lo=236, cap=256):
    """n addresses of stream 0 whose home slots lie in lo .. cap - 1: together they fill the store's end and wrap to slot 0."""
    out, a = [], 0x200000
    while len(out) < n:
        if f.home(0, a, cap) >= lo:
            out.append(a)
        a += 1
    return out


def test_fleet_store_at_its_minimum(sim):
    """256 slots, 95 planes: a probe cluster that wraps from slot 255 to slot 0 and loses its middle (every survivor is still
    found, every expired address is unknown); the same addresses in two streams with different cutoffs while the third stream
    is not selected; a reset stream's stale slots dropped by the expiry's pass."""
    rng = np.random.default_rng(71)
    f, mod = AgedFleet(sim, 3, "All Messages", "None"), FleetModel(3)
    clus = cluster_addresses(f, 30)
    shared = [0x700000 + 11 * k for k in range(25)]
    addrs = [(0, a) for a in clus] + [(0, a) for a in shared] + [(1, a) for a in shared] + [(2, a) for a in shared[:15]]
    b = [ident(a, rng) for s, a in addrs]
    t = [1000.5 + k for k in range(len(addrs))]                       # one second apart: last_seen 1000 + k ...
    for k in range(10, 20):
        t[k] = 900.5 + k                                              # ... but the cluster's middle: 910 .. 919
    ss = [s for s, a in addrs]
    S.assert_rows_equal(f.call(b, t, ss), mod.call(b, t, ss))
    assert f.stats() == dict(planes=95, capacity=256, grows=0, used=95)
    slots = [f.slot_of(0, a) for a in clus]
    assert max(slots) == 255 and min(slots) == 0 and len([x for x in slots if x < 20]) >= 5           # the cluster wraps
    check_fleet(f, mod)
    assert f.expire([950, 950, 950]) == mod.m[0].sweep(950) == 10
    check_fleet(f, mod, "the middle")
    assert f.taken() == 85 and f.stats()["used"] == 85
    assert [f.slot_of(0, a) >= 0 for a in clus] == [True] * 10 + [False] * 10 + [True] * 10
    # the same addresses in streams 0 and 1 with different cutoffs; stream 2 is not selected and keeps everything
    c0, c1 = 1000 + 40, 1000 + 55 + 12
    n = mod.m[0].sweep(c0) + mod.m[1].sweep(c1)
    assert n == 20 + 10 + 12 and f.expire([c0, c1], [0, 1]) == n
    check_fleet(f, mod, "two cutoffs")
    got = probe_all(f, mod, addrs, 2100.0, rng)
    known = (got["present"] & N.DEC_HAS_PLANE) != 0
    assert known.sum() == 95 - 10 - n and known[-15:].all() and not known[:40].any()
    # a reset stream's stale slots and an expiry in one pass
    f.reset(2)
    mod.reset(2)
    assert f.stats()["planes"] == mod.planes() and f.taken() == f.stats()["planes"] + 15
    n = mod.m[1].sweep(2200)
    assert n == 13 and f.expire([2200], [1]) == n
    assert f.taken() == f.stats()["planes"] == mod.planes() == 15     # stream 2's fifteen stale slots are gone as well
    check_fleet(f, mod, "reset and expiry")
    probe_all(f, mod, addrs, 2300.0, rng)
    b2 = [ident(a, rng) for s, a in addrs[:20]]
    S.assert_rows_equal(f.call(b2, [2400.5] * 20, [0] * 20), mod.call(b2, [2400.5] * 20, [0] * 20))     # heard again
    check_fleet(f, mod, "end")
    f.close()


def test_fleet_last_seen_survives_every_rehash(sim):
    """Growth then expiry, expiry then growth, and the renumbering rehash: last_seen moves with its slot."""
    rng = np.random.default_rng(72)
    f, mod = AgedFleet(sim, 2, "All Messages", "Conservative"), FleetModel(2, "All Messages", "Conservative")
    addr = [0x100000 + 37 * k for k in range(200)]

    def traffic(lo, hi, t0):
        pick = [(k % 2, addr[k]) for k in range(lo, hi)]
        b = [ident(a, rng) for s, a in pick]
        t = [t0 + 0.5 * k for k in range(len(pick))]
        ss = [s for s, a in pick]
        S.assert_rows_equal(f.call(b, t, ss), mod.call(b, t, ss))
    traffic(0, 100, 1000.25)
    assert f.stats()["grows"] == 0
    traffic(100, 200, 2000.25)                                          # 200 live slots: the store doubles (twice)
    assert f.stats()["grows"] >= 1 and f.stats()["capacity"] >= 512
    check_fleet(f, mod, "growth")
    n = mod.m[0].sweep(1030) + mod.m[1].sweep(2010)
    assert n > 50 and f.expire([1030, 2010]) == n
    check_fleet(f, mod, "growth then expiry")
    cap = f.stats()["capacity"]
    more = [0x900000 + 13 * k for k in range(cap // 2)]
    b, t = [ident(a, rng) for a in more], [3000.5 + 0.25 * k for k in range(len(more))]
    S.assert_rows_equal(f.call(b, t, [1] * len(more)), mod.call(b, t, [1] * len(more)))
    assert f.stats()["capacity"] > cap
    check_fleet(f, mod, "expiry then growth")
    # the renumbering rehash (the call numbers start over): announcements stay "earlier", last_seen stays
    sim.sim_fleet_set_call(f.h, ctypes.c_ulonglong(0xFFFFFFFE))
    traffic(0, 20, 4000.25)
    assert sim.sim_fleet_get_call(f.h) == 2
    check_fleet(f, mod, "renumbering")
    n = mod.m[0].sweep(4000) + mod.m[1].sweep(4000)
    assert f.expire([4000, 4000]) == n
    check_fleet(f, mod, "after the renumbering")
    probe_all(f, mod, [(k % 2, addr[k]) for k in range(0, 200, 3)], 5000.0, rng)
    check_fleet(f, mod, "end")
    f.close()


def test_fleet_no_op_expiry_and_selection_rules(sim):
    rng = np.random.default_rng(73)
    f, g_, mod = AgedFleet(sim, 3, "All Messages", "None"), AgedFleet(sim, 3, "All Messages", "None"), FleetModel(3)
    addr = [0x440000 + 5 * k for k in range(30)]
    b, t = S.mixed(rng, n=400, addresses=addr, t0=7000.5)
    ss = rng.integers(0, 3, len(b)).astype(np.int32)
    S.assert_rows_equal(f.call(b[:250], t[:250], ss[:250]), g_.call(b[:250], t[:250], ss[:250]))
    mod.call(b[:250], t[:250], ss[:250])
    before = f.snapshot()
    assert f.expire([INT64_MIN] * 3) == 0 and f.expire([1 << 62], [1][:0]) == 0         # no cutoff below; nobody selected
    after = f.snapshot()
    TP.rows_equal(before[0], after[0])
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    S.assert_rows_equal(f.call(b[250:], t[250:], ss[250:]), g_.call(b[250:], t[250:], ss[250:]))
    mod.call(b[250:], t[250:], ss[250:])
    check_fleet(f, mod)
    check_fleet(g_, mod)
    n = ctypes.c_longlong(0)
    cut = np.zeros(3, np.int64)
    for bad in ([2, 1], [0, 0], [3], [-1]):
        sel = np.array(bad, np.int32)
        assert sim.sim_exp_fleet_expire(f.h, sel.ctypes.data_as(vp), ctypes.c_int(len(sel)), cut.ctypes.data_as(vp), ctypes.c_int(1),
                                        ctypes.byref(n)) == -22
    assert sim.sim_exp_fleet_expire(f.h, None, ctypes.c_int(0), None, ctypes.c_int(1), ctypes.byref(n)) == -22
    # rows alone, last_seen alone
    a = f.snapshot()
    TP.rows_equal(f.snapshot(seen=False)[0], a[0])
    assert np.array_equal(f.snapshot(rows=False)[1], a[1])
    f.close(); g_.close()


# ---- the Python surface on the host --------------------------------------------------------------------------------------------
def test_plane_entry_with_last_seen(ge):
    rows, seen = Model("All Messages", "None"), None
    sl = TD.seq_slices(ge["seq"])[0]
    rows.rows(ge["bits"][sl][:19], ge["ts"][sl][:19])
    r, s = rows.snapshot()
    e, eseen = gold_dict(ge, "all_none", "b", 0)
    assert np.array_equal(s, eseen)
    for row, t in zip(r, s):
        d = N.plane_entry(row, np.int64(t))
        assert list(d) == ["callsign", "altitude", "speed", "heading", "vertical_rate", "latitude", "longitude", "num_msgs", "last_seen"]
        assert type(d["last_seen"]) is int and d["last_seen"] == int(t)
        plain = N.plane_entry(row)
        assert "last_seen" not in plain and list(plain) == list(d)[:-1]
    assert N.plane_entry(r[0], 0)["last_seen"] == 0 and N.plane_entry(r[0], -3)["last_seen"] == -3


class EmulatedContext:
    """What blocks.decoder asks of _native.Context, answered by the emulated kernels."""
    lib = None

    def __init__(self, fs, thr, device=0, flags=0):
        self.flags = flags
        self.filt = "All Messages"
        self.dec = None
        self.expired = []

    def set_decoder(self, msg_filter, start):
        self.dec = AgedDecoder(self.lib, msg_filter, "Conservative" if self.flags & N.FLAG_FEC_CONSERVATIVE else "None",
                               seen=bool(self.flags & N.FLAG_PLANE_AGES))

    def decode_pdus(self, bits, ts):
        return self.dec.call(bits, ts)

    def expire_planes(self, cutoff):
        assert self.flags & N.FLAG_PLANE_AGES and type(cutoff) is int
        self.expired.append(cutoff)
        return self.dec.expire(cutoff)

    def planes(self, cap=None, seen=False):
        return self.dec.snapshot() if seen else self.dec.plain_snapshot()

    def close(self):
        pass


@pytest.mark.parametrize("tag,filt,corr", CONFIGS[:2])
def test_decoder_block_with_a_plane_timeout(sim, ge, tag, filt, corr, monkeypatch, have_reference):
    """blocks.decoder(plane_timeout=60) over the emulated kernels: in front of every handled PDU the sweep
    last_seen < int(timestamp) - 60 -- the model with the same sweeps at the same points, and the reference decoder itself
    where it can be loaded; plane_dict carries last_seen.  Without plane_timeout nothing is swept and no flag is asked for."""
    from gr_adsb_amd import blocks, grshim
    EmulatedContext.lib = sim
    monkeypatch.setattr(N, "Context", EmulatedContext)
    sl = TD.seq_slices(ge["seq"])[0]
    bits, ts, snr = ge["bits"][sl], ge["ts"][sl], ge["snr"][sl]
    blk = blocks.decoder(filt, corr, plane_timeout=60)
    assert blk._ctx.flags & N.FLAG_PLANE_AGES
    mod = Model(filt, corr)
    ref = None
    if have_reference:
        import sys
        sys.path.insert(0, os.path.join(HERE, "..", "tools"))
        import make_golden_decode as G
        import ref_harness as R
        ref = R.load_reference_decoder(filt, corr, "None")
        clock = G.Clock()
        ref.decode_packet.__func__.__globals__["time"] = clock
    exp = []
    removed = 0
    for k in range(len(bits)):
        meta = {"timestamp": float(ts[k]), "snr": float(snr[k])}
        vec = np.unpackbits(bits[k])
        cutoff = int(ts[k]) - 60
        removed += mod.sweep(cutoff)
        exp.append(mod.row(bits[k], ts[k]))
        blk.decode_packet(grshim.pmt.cons(grshim.pmt.to_pmt(dict(meta)), grshim.pmt.to_pmt(vec)))
        if ref is not None:
            for key in [q for q, p in ref.plane_dict.items() if q != "" and p["last_seen"] < cutoff]:
                del ref.plane_dict[key]
            clock.now = float(ts[k])
            try:
                ref.decode_packet((dict(meta), vec.copy()))
            except Exception:
                pass
            want = {q: p for q, p in ref.plane_dict.items() if q != ""}
            have = blk.plane_dict
            assert sorted(want) == sorted(have), k
            for q, p in want.items():
                assert have[q]["last_seen"] == p["last_seen"] and have[q]["num_msgs"] == p["num_msgs"] and have[q]["callsign"] == p["callsign"]
    assert removed >= 5 and blk._ctx.expired == [int(x) - 60 for x in ts]
    pd = blk.plane_dict
    erows, eseen = mod.snapshot()
    assert list(pd) == ["{:06x}".format(int(a)) for a in erows["icao"]]
    for (key, d), row, t in zip(pd.items(), erows, eseen):
        assert d == N.plane_entry(row, t) or (np.isnan(d["latitude"]) and d["last_seen"] == int(t) and d["num_msgs"] == int(row["num_msgs"]))
    if ref is not None:
        pub = [(m["icao"], m["num_msgs"], m["callsign"]) for p, (m, _), _ in ref.msgs if p == "decoded"]
        ours = [(m["icao"], m["num_msgs"], m["callsign"]) for p, (m, _) in blk.messages if p == "decoded"]
        assert ours == pub and len(pub) > 10
    # several PDUs at once: each behind its own sweep
    blk2 = blocks.decoder(filt, corr, plane_timeout=60)
    blk2.decode_pdus([grshim.pmt.cons(grshim.pmt.to_pmt({"timestamp": float(ts[k]), "snr": 1.0}), grshim.pmt.to_pmt(np.unpackbits(bits[k])))
                      for k in range(len(bits))])
    assert blk2._ctx.expired == blk._ctx.expired and blk2.plane_dict.keys() == pd.keys()
    # the default: unchanged behaviour
    plain = blocks.decoder(filt, corr)
    assert not plain._ctx.flags & N.FLAG_PLANE_AGES and plain.plane_timeout is None
    plain.decode_pdus([grshim.pmt.cons(grshim.pmt.to_pmt({"timestamp": float(ts[k]), "snr": 1.0}), grshim.pmt.to_pmt(np.unpackbits(bits[k])))
                       for k in range(len(bits))])
    assert plain._ctx.expired == [] and all("last_seen" not in d for d in plain.plane_dict.values())
    assert len(plain.plane_dict) > len(pd)


# ---- constants, symbols, resources ---------------------------------------------------------------------------------------------
NEW_EXPORTS = ("adsb_planes_seen", "adsb_stream_planes_seen", "adsb_planes_expire", "adsb_stream_planes_expire")


def test_flag_symbols_and_abi():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_FLAG_PLANE_AGES 2048u", src) and N.FLAG_PLANE_AGES == 2048
    assert re.search(r"#define ADSB_ABI_VERSION 5\b", src) and N.ABI_VERSION == 5
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS and re.search(r"^int %s\(adsb_ctx\* ctx" % name, src, re.M), name
    for method in ("expire_planes", "expire_stream_planes"):
        assert callable(getattr(N.Context, method))
    from gr_adsb_amd import frontend
    assert callable(frontend.Receivers.expire)


def test_kernel_resources():
    """The new kernels: no scratch, no VGPR spills, no LDS, and -- but for k_ages_fold, whose loop is k_dec_fold's and as short
    of scalar registers: the last_seen pointer's two are parked in vector lanes -- no SGPR spills; k_dec_fold and k_fleet_fold
    keep none at all."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    ks = {k: v for k, v in res.items() if "k_ages_" in k}
    names = sorted(re.search(r"k_ages_[a-z_]+?(?=E)", k).group(0) for k in ks)
    assert names == ["k_ages_emit", "k_ages_expire", "k_ages_fold", "k_ages_rehash", "k_ages_store_emit"], sorted(ks)
    for k, v in list(ks.items()) + [(k, v) for k, v in res.items() if "k_dec_fold" in k or "k_fleet_fold" in k]:
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["lds_bytes_per_block"] == 0, k
        assert v["sgpr_spills"] <= (2 if "k_ages_fold" in k else 0), k
    fold = [v for k, v in res.items() if "k_dec_fold" in k][0]
    assert [v for k, v in ks.items() if "k_ages_fold" in k][0]["vgprs"] <= fold["vgprs"] + 8
