"""ADSB_FLAG_STREAM_DEDUP on the CPU: a reply heard by several receivers of a shared decoder is published once.  The emulated
kernels (tests/sim/dedup_driver.cpp: adsb_dedup_device.h's four kernels inside the shared decoder's call, the host's rule for
the carry restated) against tests/golden/g_dedup.npz -- ONE unmodified reference decoder fed the publication sequence without
the duplicates (tools/make_golden_dedup.py) -- and against the plain-Python rule of tests/dedup_replay.py; the scan across
the wavefront, workgroup and LDS-tile seams; the carry's edges; the new translation unit's build facts.

What a green run here does NOT cover: the host's own branch of fleet_step, the entry points and their refusals, and
adsb_stream_reset beside the carry -- tests/test_gpu_dedup.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import decode_streams as S
import dedup_replay as DR
import shared_replay as SR
import test_decode as TD
import test_shared_decode as TS
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
DEDUP_SO = os.path.join(SIM_DIR, "libadsb_dedup_sim.so")
CONFIGS = TD.CONFIGS
AP_BITS = N.BURST_AP_KNOWN | N.BURST_AP_FEC
TILE = 1024                   # entries per LDS tile of k_dedup_find
FS = 2e6
T0 = 1760000000.25
vp = ctypes.c_void_p


def dedup_lib():
    csrc = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, f) for f in ("dedup_driver.cpp", "shared_driver.cpp", "fleet_driver.cpp", "sim_support.h", "hipsim.h")] + \
        [os.path.join(csrc, f) for f in ("adsb_device.h", "adsb_shared_device.h", "adsb_dedup_device.h")]
    if not (os.path.exists(DEDUP_SO) and all(os.path.getmtime(DEDUP_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", DEDUP_SO])
    lib = ctypes.CDLL(DEDUP_SO)
    lib.sim_dedup_open.restype = ctypes.c_void_p
    lib.sim_dedup_fleet.restype = ctypes.c_void_p
    lib.sim_dedup_digest.restype = ctypes.c_ulonglong
    lib.sim_shared_open.restype = ctypes.c_void_p
    lib.sim_shared_digest.restype = ctypes.c_ulonglong
    lib.sim_shared_expire.restype = ctypes.c_longlong
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = dedup_lib()
    assert lib.sim_dedup_tile() == TILE
    return lib


@pytest.fixture(scope="module")
def g():
    return np.load(DR.GOLD)


def call_list(stream, n, extra_items=()):
    """(item streams, first[]) of a list whose records are grouped by stream, as SimShared.call builds them"""
    cut = np.concatenate([[0], np.flatnonzero(np.diff(stream)) + 1]).astype(np.int32) if n else np.zeros(0, np.int32)
    items = [(int(stream[c]), int(c)) for c in cut]
    for k, s in extra_items:
        items.insert(k, (s, items[k][1] if k < len(items) else n))
    assert len(set(s for s, _ in items)) == len(items), "a stream appears once per call"
    return np.array([s for s, _ in items], np.int32), np.array([f for _, f in items] + [n], np.int32)


class SimDedup:
    """A shared decoder with the de-duplication step on the emulated kernels; the carry lives in the driver."""

    def __init__(self, lib, n_streams, filt, corr, fs, starts, window, horizon, slots=1 << 16, ages=False):
        self.lib = lib
        self.h = vp(lib.sim_dedup_open(ctypes.c_int(n_streams), ctypes.c_longlong(slots), ctypes.c_int(corr == "Conservative"),
                                       ctypes.c_int(filt == "All Messages"), ctypes.c_int(ages), ctypes.c_double(fs),
                                       ctypes.c_double(window), ctypes.c_double(horizon)))
        self.fleet = vp(lib.sim_dedup_fleet(self.h))
        for s, t in enumerate(starts):
            lib.sim_shared_set_start(self.fleet, ctypes.c_int(s), ctypes.c_double(t))

    def close(self):
        self.lib.sim_dedup_close(self.h)

    def call(self, bits14, offset, stream, grid=3, dem=None, extra_items=(), rc=0):
        """-> (flags, rows, order, ts, dup), everything at list positions"""
        b = np.ascontiguousarray(bits14, dtype=np.uint8)
        off = np.ascontiguousarray(offset, dtype=np.int64)
        stream = np.asarray(stream, dtype=np.int32)
        n = len(b)
        ist, first = call_list(stream, n, extra_items)
        d = None if dem is None else np.ascontiguousarray(dem, dtype=np.uint8)
        flags, rows = np.zeros(n, np.uint16), np.zeros(n, dtype=N.DECODED_DTYPE)
        order, ts, dup = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
        got = self.lib.sim_dedup_call(self.h, b.ctypes.data_as(vp), off.ctypes.data_as(vp), None if d is None else d.ctypes.data_as(vp),
                                      ctypes.c_int(n), ist.ctypes.data_as(vp), first.ctypes.data_as(vp), ctypes.c_int(len(ist)),
                                      ctypes.c_int(grid), flags.ctypes.data_as(vp), rows.ctypes.data_as(vp), order.ctypes.data_as(vp),
                                      ts.ctypes.data_as(vp), dup.ctypes.data_as(vp))
        assert got == rc, "guard (-1), bad key or order (-2), error word / books (-3), refused (-4), argument (-5), carry (-6): %d" % got
        return flags, rows, order, ts, dup

    def reset(self):
        self.lib.sim_dedup_reset(self.h)

    def digest(self):
        return int(self.lib.sim_dedup_digest(self.h))

    def stats(self):
        d, c, hi = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
        self.lib.sim_dedup_stats(self.h, ctypes.byref(d), ctypes.byref(c), ctypes.byref(hi))
        return d.value, c.value, hi.value

    def carry(self):
        """(ts, stream, marker) of the carry's entries, in its order"""
        cap = self.stats()[1]
        ts, st, mk = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        assert self.lib.sim_dedup_carry(self.h, ts.ctypes.data_as(vp), st.ctypes.data_as(vp), mk.ctypes.data_as(vp), ctypes.c_int(cap)) == cap
        return ts, st, mk

    def set_max_cap(self, cap):
        self.lib.sim_shared_set_max_cap(self.fleet, ctypes.c_longlong(cap))

    def fleet_stats(self):
        v = [ctypes.c_longlong() for _ in range(4)]
        self.lib.sim_shared_stats(self.fleet, *[ctypes.byref(x) for x in v])
        return dict(planes=v[0].value, capacity=v[1].value, grows=v[2].value, used=v[3].value)

    def planes(self):
        cap = 1 << 16
        addr, seen = np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        n = self.lib.sim_shared_planes(self.fleet, addr.ctypes.data_as(vp), seen.ctypes.data_as(vp), ctypes.c_int(cap))
        return dict(zip(addr[:n].tolist(), seen[:n].tolist()))


def check_call(got, exp, bits14, fec=False, dem=None):
    """One call of the emulation against the replay's: order, dup, the verdict flags, every row."""
    fl, r, order, _, dup = got
    efl, er, eorder, edup = exp
    assert np.array_equal(order, eorder)
    assert np.array_equal(dup, edup), (np.flatnonzero(dup != edup)[:5], dup[dup != edup][:5], edup[dup != edup][:5])
    live = np.ones(len(fl), bool) if dem is None else np.asarray(dem, bool)
    assert np.array_equal((fl & AP_BITS)[live], efl[live])
    assert ((fl & N.BURST_DEMOD) != 0).tolist() == live.tolist()                # a duplicate keeps ADSB_BURST_DEMOD
    assert not (fl[dup != -1] & AP_BITS).any()
    if live.any():
        S.assert_rows_equal(r[live], DR.rows_of(er, bits14, edup, fec)[live])


# ---- the golden ------------------------------------------------------------------------------------------------------------
def golden_calls(g, partition):
    return SR.golden_calls(g, partition)


def test_golden_holds_the_cases(g):
    """Cases (a) to (i) of tools/make_golden_dedup.py, from the file alone."""
    ts, stream, call = g["ts"], g["stream"], g["call"]
    w, hz = float(g["window"]), float(g["horizon"])
    assert w == 2.0 ** -9 and hz == 4.0 and set(stream.tolist()) == {0, 1, 2, 3} and 200 <= len(ts) <= 400
    assert np.array_equal(ts, g["start"][stream] + g["offset"].astype(np.float64) / float(g["fs"]))
    assert np.spacing(ts.max()) == 2.0 ** -22
    p = {k[5:]: int(g[k]) for k in g.files if k.startswith("case_")}
    first = np.array([np.flatnonzero(call == c)[0] for c in range(call.max() + 1)])
    for e in ("none", "cons"):
        d = g["dup_" + e]
        absd = np.where(d >= 0, d + first[call], d)
        tag = "all_" + e
        nm, has = g["nmsgs_" + tag], g["has_" + tag]
        assert np.array_equal(g["port_" + tag] == 4, d != -1)
        # (a)
        assert {stream[p["a0"]], stream[p["a1"]], stream[p["a2"]]} == {0, 1, 2} and absd[p["a1"]] == absd[p["a2"]] == p["a0"]
        assert d[p["a0"]] == -1 and nm[p["a0"]] == 1 and max(ts[p[k]] for k in ("a0", "a1", "a2")) - ts[p["a0"]] <= w
        # (b)
        assert [stream[p[k]] for k in ("b_e0", "b_e1", "b_o0", "b_o1")] == [0, 2, 1, 3]
        assert absd[p["b_e1"]] == p["b_e0"] and absd[p["b_o1"]] == p["b_o0"] and nm[p["b_o0"]] == 2
        assert not np.isnan(g["lat_" + tag].view(np.float64)[p["b_o0"]])
        # (c)
        assert ts[p["c_dup"]] - ts[p["c_q"]] == w and absd[p["c_dup"]] == p["c_q"]
        assert ts[p["c_not"]] == np.nextafter(ts[p["c_q2"]] + w, np.inf) and d[p["c_not"]] == -1 and nm[p["c_not"]] == 2
        assert g["bits"][p["c_not"]].tobytes() == g["bits"][p["c_q2"]].tobytes() and stream[p["c_not"]] != stream[p["c_q2"]]
        # (d)
        assert stream[p["d0"]] == stream[p["d1"]] and g["bits"][p["d0"]].tobytes() == g["bits"][p["d1"]].tobytes()
        assert ts[p["d1"]] - ts[p["d0"]] <= w and d[p["d0"]] == d[p["d1"]] == -1 and nm[p["d1"]] == 2
        # (e)
        b = g["bits"]
        assert b[p["e_q"]][0] >> 3 == 11 and b[p["e_q"]][:7].tobytes() == b[p["e_dup"]][:7].tobytes()
        assert b[p["e_q"]][7:].tobytes() != b[p["e_dup"]][7:].tobytes() and absd[p["e_dup"]] == p["e_q"]
        assert b[p["e_q2"]][0] >> 3 == 17 and b[p["e_q2"]][:13].tobytes() == b[p["e_not"]][:13].tobytes() and d[p["e_not"]] == -1
        # (f)
        assert call[p["f_dup"]] > call[p["f_q"]] and ts[p["f_dup"]] < ts[p["f_q"]] and d[p["f_dup"]] == -2
        # (g)
        assert call[p["g_again"]] > call[p["g_q"]] and abs(ts[p["g_again"]] - ts[p["g_q"]]) <= w
        assert ts[call < call[p["g_again"]]].max() - ts[p["g_q"]] > hz and d[p["g_again"]] == -1 and nm[p["g_again"]] == 2
        # (h)
        assert b[p["h_q"]][0] >> 3 == 4 and absd[p["h_dup"]] == p["h_q"] and has[p["h_q"]] == 0
        assert absd[p["h_ann_dup"]] == p["h_ann"] and nm[p["h_ann"]] == 1 and has[p["h_known"]] == 1 and nm[p["h_known"]] == 2
        # (i)
        assert call[p["i_dup1"]] == call[p["i_dup2"]] > call[p["i_q"]] and d[p["i_dup1"]] == d[p["i_dup2"]] == -2
        assert abs(ts[p["i_dup2"]] - ts[p["i_dup1"]]) <= w and stream[p["i_dup1"]] != stream[p["i_dup2"]]
    # a repaired hearing is a duplicate of the clean one only where the decoder repairs
    assert g["dup_none"][p["fec_dup"]] == -1 and g["dup_cons"][p["fec_dup"]] >= 0
    assert any(len(g["items_%d" % c]) > len(set(stream[call == c].tolist())) for c in range(call.max() + 1))


def golden_dup(g, corr):
    return g["dup_cons" if corr == "Conservative" else "dup_none"]


def check_golden(rows, dup, g, tag, corr):
    gd = golden_dup(g, corr)
    assert np.array_equal(dup != -1, gd != -1)
    keep = np.flatnonzero(gd == -1)
    TD.check_rows(rows[keep], g, tag, keep)
    assert (rows["port"][gd != -1] == N.DEC_DUPLICATE).all() and not rows["present"][gd != -1].any()


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_replay_equals_golden(g, tag, filt, corr):
    rep = DR.Replay(filt, corr, float(g["window"]), float(g["horizon"]))
    n = len(g["ts"])
    rows, dup = np.zeros(n, dtype=N.DECODED_DTYPE), np.zeros(n, np.int32)
    for idx, _ in golden_calls(g, 0):
        _, er, _, d = rep.call(g["bits"][idx], g["ts"][idx], g["stream"][idx])
        rows[idx], dup[idx] = DR.rows_of(er, g["bits"][idx], d, rep.fec), d
    assert np.array_equal(dup, golden_dup(g, corr))
    check_golden(rows, dup, g, tag, corr)
    planes = {a: t for a, t in zip(g["f_icao_" + tag].tolist(), g["f_seen_" + tag].tolist()) if a >= 0}
    assert rep.rep.seen == planes


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("partition", [0, 1])
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_emulated_kernels_equal_golden(sim, g, tag, filt, corr, partition, grid):
    """The golden's calls (and each cut in two by time) through the emulated kernels, with one and with three workgroups:
    against the reference's rows and byte for byte against the replay's."""
    w, hz = float(g["window"]), float(g["horizon"])
    f = SimDedup(sim, 4, filt, corr, float(g["fs"]), g["start"].tolist(), w, hz, slots=0, ages=True)
    rep = DR.Replay(filt, corr, w, hz)
    n = len(g["ts"])
    rows, dup = np.zeros(n, dtype=N.DECODED_DTYPE), np.zeros(n, np.int32)
    for idx, extra in golden_calls(g, partition):
        got = f.call(g["bits"][idx], g["offset"][idx], g["stream"][idx], grid=grid, extra_items=extra)
        assert got[3].tobytes() == g["ts"][idx].tobytes()
        exp = rep.call(g["bits"][idx], g["ts"][idx], g["stream"][idx])
        check_call(got, exp, g["bits"][idx], rep.fec)
        rows[idx], dup[idx] = got[1], got[4]
        assert f.stats() == rep.stats()
    if partition == 0:
        assert np.array_equal(dup, golden_dup(g, corr))
    check_golden(rows, dup, g, tag, corr)
    planes = {a: t for a, t in zip(g["f_icao_" + tag].tolist(), g["f_seen_" + tag].tolist()) if a >= 0}
    assert f.planes() == planes and f.fleet_stats()["planes"] == len(planes)
    f.close()


# ---- the scan across the seams ---------------------------------------------------------------------------------------------
IDENT = np.packbits(S.es(0x4B1A01, 4, np.concatenate([S.ib(5, 3), np.tile(S.ib(9, 6), 8)])))      # a DF 17 identification


def one_reply(n):
    """(bits, offset, stream): one reply heard by n streams, stream s at sample 1000 + s (0.5 us apart: all within 2 ms)"""
    return np.tile(IDENT, (n, 1)), 1000 + np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int32)


@pytest.mark.parametrize("n", [2, 65, 257, TILE + 1])
def test_one_reply_heard_by_many_streams(sim, n):
    """One reply heard by n receivers -- a wavefront and one, a workgroup and one, an LDS tile and one: exactly one hearing is
    published and dup[] names it, in one call; with the first hearing in an earlier call every later one is -2; and against a
    carry of n - 1 hearings the one that arrives last is -2."""
    b, off, s = one_reply(n)
    starts = [T0] * n
    f = SimDedup(sim, n, "All Messages", "None", FS, starts, 0.002, 1.0)
    fl, r, order, _, dup = f.call(b, off, s, grid=3)
    assert np.array_equal(order, np.arange(n)) and dup[0] == -1 and (dup[1:] == 0).all()
    assert r["num_msgs"][0] == 1 and (r["port"][1:] == N.DEC_DUPLICATE).all() and set(f.planes()) == {0x4B1A01}
    assert f.stats()[:2] == (n - 1, n)
    f.close()
    f = SimDedup(sim, n, "All Messages", "None", FS, starts, 0.002, 1.0)
    assert f.call(b[:1], off[:1], s[:1])[4].tolist() == [-1]
    rev = np.arange(1, n)[::-1]                                        # the items in descending stream order: the list is not the time order
    fl, r, order, _, dup = f.call(b[rev], off[rev], s[rev], grid=2)
    assert (dup == -2).all() and np.array_equal(order, np.arange(n - 1)[::-1]) and f.stats()[:2] == (n - 1, n)
    f.close()
    f = SimDedup(sim, n, "All Messages", "None", FS, starts, 0.002, 1.0)
    assert (f.call(b[1:], off[1:], s[1:])[4][1:] == 0).all()
    fl, r, _, _, dup = f.call(b[:1], off[:1], s[:1], grid=1)           # n = 1 against a carry, and EARLIER in time than all of it
    assert dup.tolist() == [-2] and r["port"][0] == N.DEC_DUPLICATE and fl[0] & N.BURST_DEMOD
    ts, st, mk = f.carry()
    assert st.tolist() == list(range(n)) and (mk == 2).all() and np.all(np.diff(ts) >= 0)
    f.close()


def fillers(n, seed):
    """n distinct payloads that match nothing: DF 17 with random bytes (they fail parity and publish nothing, but take part)"""
    b = np.random.default_rng(seed).integers(0, 256, (n, 14)).astype(np.uint8)
    b[:, 0] = 0x8D
    b[:, 1:4] = np.array([[k >> 16, (k >> 8) & 255, k & 255] for k in range(n)], np.uint8)      # distinct, whatever the rest
    return b


def seam_world(front, between):
    """One reply's hearings among fillers, everything inside one 2 ms window (one sample apart).  In time order: a decoy --
    the reply on stream 1 itself --, `front` fillers, the hearing A on stream 0, a second hearing A2 on stream 3, `between`
    fillers, and B on stream 1.  B's earliest match is A, at place front + 1 of the staged range: with front > TILE that is
    in the second tile, which is a partial one, and the decoy in the first tile must not count (the same stream).
    -> (bits, offset, stream) grouped by stream, and the list positions of decoy, A, A2, B"""
    n = front + between + 4
    assert n < 3900                                                    # 0.002 s are 4000 samples
    who = np.full(n, 2, np.int32)                                      # the fillers are stream 2's
    bits = fillers(n, front)
    for place, s_ in ((0, 1), (front + 1, 0), (front + 2, 3), (n - 1, 1)):
        who[place], bits[place] = s_, IDENT
    off = 1000 + np.arange(n, dtype=np.int64)
    order = np.argsort(who, kind="stable")                             # the list: grouped by stream, each in time order
    at = {int(p): k for k, p in enumerate(order)}
    return bits[order], off[order], who[order], [at[0], at[front + 1], at[front + 2], at[n - 1]]


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("front,between", [(TILE + 76, 5), (TILE + 300, 260), (2 * TILE + 9, 1)])
def test_the_earliest_match_lies_in_a_later_partial_tile(sim, front, between, grid):
    """The in-call range and the carry range of k_dedup_find beyond one LDS tile: the match is staged at tb > q_lo, in a
    partial last tile (also two tiles on, and with B's workgroup starting behind A).  dup[] against the replay, and by name."""
    b, off, s, (decoy, a, a2, bb) = seam_world(front, between)
    n = len(b)
    starts = [T0] * 4
    # in one call
    f, rep = SimDedup(sim, 4, "All Messages", "None", FS, starts, 0.002, 1.0), DR.Replay("All Messages", "None", 0.002, 1.0)
    got = f.call(b, off, s, grid=grid)
    check_call(got, rep.call(b, got[3], s), b)
    dup = got[4]
    assert dup[decoy] == -1 and dup[a] == decoy and dup[a2] == decoy and dup[bb] == a          # B's own stream's decoy does not count
    assert (np.delete(dup, [a, a2, bb]) == -1).all() and got[1]["num_msgs"][decoy] == 1
    f.close()
    # against the carry: everything but B delivered first; then B, and beside it a hearing EARLIER than all of the carry
    f, rep = SimDedup(sim, 5, "All Messages", "None", FS, starts + [T0], 0.002, 1.0), DR.Replay("All Messages", "None", 0.002, 1.0)
    head = np.delete(np.arange(n), bb)
    got = f.call(b[head], off[head], s[head], grid=grid)
    check_call(got, rep.call(b[head], got[3], s[head]), b[head])
    tail_b, tail_off, tail_s = np.array([IDENT, b[bb]]), np.array([900, off[bb]], np.int64), np.array([4, 1], np.int32)
    got = f.call(tail_b, tail_off, tail_s, grid=grid)
    check_call(got, rep.call(tail_b, got[3], tail_s), tail_b)
    assert got[4].tolist() == [-2, -2] and f.stats() == rep.stats() and f.stats()[1] == n + 1
    # ... and when the carry's only other-stream hearing is A (the decoy's and A2's streams are B's own): still found, in tile 2
    f.close()
    f, rep = SimDedup(sim, 4, "All Messages", "None", FS, starts, 0.002, 1.0), DR.Replay("All Messages", "None", 0.002, 1.0)
    s2 = s.copy()
    s2[a2] = 1
    order2 = np.argsort(s2[head], kind="stable")
    h2 = head[order2]
    got = f.call(b[h2], off[h2], s2[h2], grid=grid)
    check_call(got, rep.call(b[h2], got[3], s2[h2]), b[h2])
    got = f.call(b[[bb]], off[[bb]], s2[[bb]], grid=grid)
    check_call(got, rep.call(b[[bb]], got[3], s2[[bb]]), b[[bb]])
    assert got[4].tolist() == [-2]
    f.close()


@pytest.mark.parametrize("grid", [1, 3])
def test_more_than_two_tiles_of_hearings(sim, grid):
    """2 * TILE + 10 hearings of one reply on stream 1 (one transmitter heard over and over: all published), ONE on stream 0
    behind them, forty more on stream 1: the one on stream 0 names the first of stream 1's, the forty name the one on stream
    0 -- their only match, two tiles into the range."""
    k = 2 * TILE + 10
    n = k + 41
    b = np.tile(IDENT, (n, 1))
    who = np.ones(n, np.int32)
    who[k] = 0
    off = 1000 + np.arange(n, dtype=np.int64)
    order = np.argsort(who, kind="stable")
    b, off, s = b[order], off[order], who[order]                       # the list: stream 0's one record first
    f, rep = SimDedup(sim, 2, "All Messages", "None", FS, [T0, T0], 0.002, 1.0), DR.Replay("All Messages", "None", 0.002, 1.0)
    got = f.call(b, off, s, grid=grid)
    check_call(got, rep.call(b, got[3], s), b)
    dup = got[4]
    assert dup[0] == 1 and (dup[1:k + 1] == -1).all() and (dup[k + 1:] == 0).all() and got[1]["num_msgs"][k] == k
    f.close()


def test_all_timestamps_equal(sim):
    """Bit-equal timestamps: the list order is the publication order, the first hearing is published, and window = 0 accepts
    exactly these."""
    n = 300
    b, _, s = one_reply(n)
    off = np.full(n, 5000, np.int64)
    for window in (0.002, 0.0):
        f = SimDedup(sim, n, "All Messages", "None", FS, [T0] * n, window, 1.0)
        dup = f.call(b, off, s)[4]
        assert dup[0] == -1 and (dup[1:] == 0).all()
        f.close()


def test_window_zero(sim):
    """window = 0: only bit-equal timestamps match -- one sample apart is another transmission."""
    b, _, s = one_reply(4)
    off = np.array([5000, 5000, 5001, 5001], np.int64)
    f = SimDedup(sim, 4, "All Messages", "None", FS, [T0] * 4, 0.0, 1.0)
    rep = DR.Replay("All Messages", "None", 0.0, 1.0)
    got = f.call(b, off, s)
    check_call(got, rep.call(b, got[3], s), b)
    assert got[4].tolist() == [-1, 0, -1, 2] and got[1]["num_msgs"].tolist() == [1, 0, 2, 0]
    got = f.call(b[:2], np.array([5001, 5002], np.int64), s[:2])       # stream 0 at 5001: streams 2 and 3 were there; stream 1 at 5002: nobody
    assert got[4].tolist() == [-2, -1]
    f.close()


def test_records_without_a_pdu_and_the_horizon(sim):
    """A call of records without ADSB_BURST_DEMOD marks nothing and still moves hi; a call whose records all lie behind
    hi - horizon leaves the carry as it was; the cut drops what hi has left behind."""
    b, _, s = one_reply(3)
    f = SimDedup(sim, 3, "All Messages", "None", FS, [T0] * 3, 0.002, 1.0)
    rep = DR.Replay("All Messages", "None", 0.002, 1.0)
    sec = int(FS)

    def both(idx, off, dem=None):
        got = f.call(b[idx], np.asarray(off, np.int64), s[idx], dem=dem)
        exp = rep.call(b[idx], got[3], s[idx], dem=dem)
        check_call(got, exp, b[idx], dem=dem)
        assert f.stats() == rep.stats()
        return got
    both([0, 1], [1000, 1400])
    assert f.stats()[:2] == (1, 2)
    got = both([0, 1, 2], [1800, 1900, 2000], dem=[0, 0, 0])           # nobody takes part
    assert (got[4] == -1).all() and not got[1]["port"].any() and f.carry()[2].tolist() == [2, 2, 0, 0, 0]
    got = both([2], [3 * sec], dem=[0])                                # hi moves two seconds on: the carry empties but for this record
    assert f.stats()[1:] == (1, T0 + 3.0) and f.carry()[2].tolist() == [0]
    before = f.carry()
    got = both([0, 1], [sec, sec + 200])                               # behind the horizon: merged and cut at once, but still a pair
    assert got[4].tolist() == [-1, 0] and f.stats()[1] == 1 and f.carry()[0].tobytes() == before[0].tobytes()
    got = both([2], [sec + 400])                                       # ... that nobody remembers
    assert got[4].tolist() == [-1]
    f.close()


def test_merge_with_ties_on_both_sides(sim):
    """The carry's merge is stable and puts the carry first on equal keys: four calls at the same two timestamps."""
    n = 6
    b, _, s = one_reply(n)
    f = SimDedup(sim, n, "All Messages", "None", FS, [T0] * n, 0.002, 1.0)
    f.call(b[[0, 1]], np.array([4000, 6000], np.int64), s[[0, 1]])
    f.call(b[[2, 3]], np.array([6000, 4000], np.int64), s[[2, 3]])
    f.call(b[[5, 4]], np.array([4000, 6000], np.int64), s[[5, 4]])
    ts, st, _ = f.carry()
    assert st.tolist() == [0, 3, 5, 1, 2, 4] and np.array_equal(ts, T0 + np.array([4000] * 3 + [6000] * 3) / FS)
    f.call(b[[0]], np.array([5000], np.int64), s[[0]])
    assert f.carry()[1].tolist() == [0, 3, 5, 0, 1, 2, 4]
    f.close()


def test_one_stream_is_the_shared_decoder(sim):
    """A context with one stream never marks anything: flags, rows and order are byte for byte the shared emulation's."""
    b, t = S.mixed(np.random.default_rng(21), n=300, addresses=TS.FLEET[:20], t0=0.0, dt=(0.0002, 0.003))
    b[1::2] = b[0::2]                                                  # every reply twice, inside the window
    off, s = np.round(t * FS).astype(np.int64), np.zeros(len(b), np.int32)
    f = SimDedup(sim, 1, "All Messages", "Conservative", FS, [T0], 0.002, 1.0)
    plain = TS.SimShared(sim, 1, "All Messages", "Conservative", FS, [T0])
    for lo in range(0, len(b), 120):
        sl = slice(lo, lo + 120)
        fl, r, order, ts, dup = f.call(b[sl], off[sl], s[sl])
        pfl, pr, porder, pts = plain.call(b[sl], off[sl], s[sl])
        assert (dup == -1).all() and fl.tobytes() == pfl.tobytes() and r.tobytes() == pr.tobytes() and np.array_equal(order, porder)
    assert f.stats()[0] == 0 and int(sim.sim_shared_digest(f.fleet)) == plain.digest()
    f.close(), plain.close()


# ---- random fleets ---------------------------------------------------------------------------------------------------------
def random_fleet(seed, n_streams=5, n_replies=150):
    """Replies 5 ms apart, each heard by a random subset of the streams up to 0.9 ms late: hearings of one reply lie pairwise
    within the 2 ms window, those of different replies never.  -> (bits, offset, stream, cluster), grouped by stream, and the
    streams' starts (a few samples apart, so that timestamps tie and cross)"""
    rng = np.random.default_rng(seed)
    b, _ = S.mixed(rng, n=n_replies, addresses=TS.FLEET[:12], t0=0.0, dt=(0.001, 0.002))
    starts = [T0 + k * 2.0 ** -20 for k in range(n_streams)]
    rows = []
    for k in range(n_replies):
        hear = np.flatnonzero(rng.random(n_streams) < 0.6)
        for s in hear:
            bits = b[k].copy()
            if bits[0] >> 3 in (0, 4, 5, 11):
                bits[7:] = rng.integers(0, 256, 7)
            rows.append((int(s), int(round((0.01 + 0.005 * k) * FS)) + int(rng.integers(0, 1800)), bits, k))
    rows.sort(key=lambda r: (r[0], r[1]))
    return (np.array([r[2] for r in rows], np.uint8), np.array([r[1] for r in rows], np.int64), np.array([r[0] for r in rows], np.int32),
            np.array([r[3] for r in rows], np.int32), starts)


def random_calls(rng, off, stream, n_streams):
    """A chunking: every stream delivers its records in order, in calls whose boundaries jitter by +-20 ms per stream."""
    at = [0] * n_streams
    idx = [np.flatnonzero(stream == s) for s in range(n_streams)]
    t = 0.0
    while any(at[s] < len(idx[s]) for s in range(n_streams)):
        t += float(rng.uniform(0.03, 0.15))
        parts = []
        for s in rng.permutation(n_streams):
            lim = (t + float(rng.uniform(-0.02, 0.02))) * FS
            k = at[s]
            while k < len(idx[s]) and off[idx[s][k]] < lim:
                k += 1
            if k > at[s] and rng.random() < 0.85:
                parts.append(idx[s][at[s]:k])
                at[s] = k
        if parts:
            yield np.concatenate(parts)


def fleet_under_chunkings(sim, b, off, stream, cluster, starts, corr, chunk_seeds):
    """The emulation is the replay call by call, and of every reply's hearings exactly one is published whatever the chunking."""
    for seed in chunk_seeds:
        f = SimDedup(sim, len(starts), "All Messages", corr, FS, starts, 0.002, 1.0, slots=0)
        rep = DR.Replay("All Messages", corr, 0.002, 1.0)
        dup = np.zeros(len(b), np.int32)
        for k, idx in enumerate(random_calls(np.random.default_rng(seed), off, stream, len(starts))):
            got = f.call(b[idx], off[idx], stream[idx], grid=1 + k % 3)
            check_call(got, rep.call(b[idx], got[3], stream[idx]), b[idx], rep.fec)
            dup[idx] = got[4]
        assert f.stats() == rep.stats()
        published = np.bincount(cluster[dup == -1], minlength=cluster.max() + 1)
        assert (published[np.unique(cluster)] == 1).all()
        f.close()


def test_a_seeded_fleet_with_repairs(sim):
    """150 replies to five receivers, Conservative, three chunkings (the larger, fixed companion of the property below)."""
    b, off, stream, cluster, starts = random_fleet(2)
    fleet_under_chunkings(sim, b, off, stream, cluster, starts, "Conservative", [200, 201, 202])


_pool = {}


def reply_pool():
    """48 replies of six aircraft: few enough that the same payload (an identification) comes back in later clusters"""
    if "b" not in _pool:
        _pool["b"] = S.mixed(np.random.default_rng(31), n=48, addresses=TS.FLEET[:6], t0=0.0, dt=(0.001, 0.002))[0]
    return _pool["b"]


@st.composite
def fleets(draw):
    """Replies 5 ms apart, each a member of reply_pool() heard by a non-empty subset of 2 .. 6 receivers 0 .. 1800 samples
    late (pairwise within the 2 ms window; different replies never are); starts a few ulps apart or equal; three chunkings."""
    n_streams = draw(st.integers(2, 6))
    replies = draw(st.lists(st.tuples(st.integers(0, 47), st.dictionaries(st.integers(0, n_streams - 1), st.integers(0, 1800), min_size=1)),
                            min_size=1, max_size=60))
    skew = draw(st.sampled_from([0.0, 2.0 ** -22, 2.0 ** -20]))
    corr = draw(st.sampled_from(["None", "Conservative"]))
    chunk_seeds = draw(st.tuples(st.integers(0, 2 ** 31), st.integers(0, 2 ** 31), st.integers(0, 2 ** 31)))
    return n_streams, replies, skew, corr, chunk_seeds


@settings(max_examples=20, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
@given(fleets())
def test_random_fleets(sim, world):
    """Property: device = replay for every call, and the published count of every reply is 1, under three random chunkings."""
    n_streams, replies, skew, corr, chunk_seeds = world
    pool, tails = reply_pool(), np.random.default_rng(len(replies))
    rows = []
    for k, (which, hear) in enumerate(replies):
        for s_, late in hear.items():
            bits = pool[which].copy()
            if bits[0] >> 3 in (0, 4, 5, 11):
                bits[7:] = tails.integers(0, 256, 7)
            rows.append((s_, int(round((0.01 + 0.005 * k) * FS)) + late, bits, k))
    rows.sort(key=lambda r: (r[0], r[1]))
    b, off = np.array([r[2] for r in rows], np.uint8), np.array([r[1] for r in rows], np.int64)
    stream, cluster = np.array([r[0] for r in rows], np.int32), np.array([r[3] for r in rows], np.int32)
    fleet_under_chunkings(sim, b, off, stream, cluster, [T0 + k * skew for k in range(n_streams)], corr, chunk_seeds)


# ---- the host's rules, restated in the driver ------------------------------------------------------------------------------
def test_a_refused_call_changes_nothing(sim):
    """A call the store has no room for is refused: the store, the carry, hi and the count keep their digest, and the call,
    repeated with room, gives the bytes of a run that was never refused."""
    b, off, stream, _, starts = random_fleet(7, n_replies=300)
    cuts = [0, int(0.1 * FS), int(0.6 * FS), int(0.9 * FS), 1 << 40]           # the first call fits the 256 slots, the second does not
    calls = [np.flatnonzero((off >= lo) & (off < hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    clean = SimDedup(sim, len(starts), "All Messages", "None", FS, starts, 0.002, 1.0, slots=0)
    want = [clean.call(b[i], off[i], stream[i]) for i in calls]
    f = SimDedup(sim, len(starts), "All Messages", "None", FS, starts, 0.002, 1.0, slots=0)
    got = [f.call(b[calls[0]], off[calls[0]], stream[calls[0]])]
    f.set_max_cap(f.fleet_stats()["capacity"])
    k = 1
    assert 2 * (f.fleet_stats()["used"] + len(calls[k])) > f.fleet_stats()["capacity"] and f.stats()[0] > 0
    before, stats = f.digest(), f.stats()
    f.call(b[calls[k]], off[calls[k]], stream[calls[k]], rc=-4)
    assert f.digest() == before and f.stats() == stats
    f.set_max_cap(1 << 27)
    got += [f.call(b[i], off[i], stream[i]) for i in calls[k:]]
    for gg, ww in zip(got, want):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(gg, ww))
    assert f.digest() == clean.digest()
    f.close(), clean.close()


def test_decoder_reset_clears_the_carry_and_a_stream_reset_does_not(sim):
    b, off, s = one_reply(3)
    f = SimDedup(sim, 3, "All Messages", "None", FS, [T0] * 3, 0.002, 1.0)
    assert f.call(b[:2], off[:2], s[:2])[4].tolist() == [-1, 0] and f.stats() == (1, 2, T0 + 1001 / FS)
    before = f.digest()
    for stream in (0, 1, 2):                                           # adsb_stream_reset: framing only, also for index 0
        sim.sim_dedup_stream_reset(f.h, ctypes.c_int(stream))
    assert f.digest() == before and f.stats() == (1, 2, T0 + 1001 / FS)
    f.reset()
    assert f.stats() == (0, 0, 0.0) and f.planes() == {}
    fl, r, _, _, dup = f.call(b[2:], off[2:], s[2:])                   # the third hearing: nobody remembers the first two
    assert dup.tolist() == [-1] and r["num_msgs"][0] == 1 and f.stats()[:2] == (0, 1)
    f.close()


def test_a_duplicate_does_not_move_last_seen(sim):
    """ADSB_FLAG_PLANE_AGES: the second hearing arrives in the next whole second and leaves the plane's clock alone."""
    b, _, s = one_reply(2)
    f = SimDedup(sim, 2, "All Messages", "None", FS, [T0, T0], 0.002, 1.0, ages=True)
    edge = int(0.75 * FS)                                              # T0 + 0.75 s: the next whole second
    assert f.call(b[:1], np.array([edge - 100], np.int64), s[:1])[4].tolist() == [-1]
    assert f.planes() == {0x4B1A01: int(T0)}
    fl, r, _, ts, dup = f.call(b[1:], np.array([edge + 100], np.int64), s[1:])
    assert int(ts[0]) == int(T0) + 1 and dup.tolist() == [-2]
    assert f.planes() == {0x4B1A01: int(T0)} and f.fleet_stats()["planes"] == 1
    f.close()


# ---- build facts -----------------------------------------------------------------------------------------------------------
def test_kernel_resources_dedup(sim):
    """The third translation unit's report: exactly the four k_dedup_* kernels, none with scratch or spills; k_dedup_find's LDS
    is the tile DESIGN.md §3h states (1024 entries of 16 bytes and the three bounds), the others use none; the other two
    units keep their kernel sets."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES_DEDUP))
    name = lambda k: re.search(r"k_dedup_[a-z_]+?(?=E)", k).group(0)      # noqa: E731
    assert sorted(name(k) for k in res) == ["k_dedup_entries", "k_dedup_find", "k_dedup_mark", "k_dedup_merge"], sorted(res)
    for k, v in res.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    lds = {name(k): v["lds_bytes_per_block"] for k, v in res.items()}
    assert lds["k_dedup_find"] == TILE * 16 + 16 == sim.sim_dedup_lds_bytes()
    assert lds["k_dedup_entries"] == lds["k_dedup_merge"] == lds["k_dedup_mark"] == 0
    design = open(os.path.join(HERE, "..", "DESIGN.md")).read()
    assert "%d bytes of LDS" % (TILE * 16 + 16) in design
    shared, main = json.load(open(B.RES_SHARED)), json.load(open(B.RES))
    assert len(shared) == 6 and all("k_shared_" in k for k in shared)
    assert not any("k_dedup" in k or "k_shared" in k for k in main) and not any("k_dedup" in k for k in shared)
    assert B.SOURCES == ["adsb_hip.hip"] and B.SHARED_SOURCE == "adsb_shared.hip" and B.DEDUP_SOURCE == "adsb_dedup.hip"
    assert all(d in B.DEPS for d in ("adsb_dedup.hip", "adsb_dedup.h", "adsb_dedup_device.h"))


def test_flag_constant_and_export_names():
    hdr = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_FLAG_STREAM_DEDUP (\d+)u", hdr).group(1) == str(N.FLAG_STREAM_DEDUP) == "8192"
    assert re.search(r"#define ADSB_DEC_DUPLICATE (\d+)u", hdr).group(1) == str(N.DEC_DUPLICATE) == "4"
    assert re.search(r"#define ADSB_ABI_VERSION (\d+)", hdr).group(1) == "5" and N.ABI_VERSION == 5
    for name in ("adsb_streams_set_dedup", "adsb_stream_last_duplicates", "adsb_stream_dedup_stats"):
        assert name in N.EXPORTS and re.search(r"^int %s\(" % name, hdr, re.M)
    for name in ("set_streams_dedup", "last_stream_duplicates", "stream_dedup_stats"):
        assert callable(getattr(N.Context, name))
    assert "NOT DONE" not in hdr and "is the follow-up" not in hdr
