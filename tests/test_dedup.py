"""ADSB_FLAG_STREAM_DEDUP on the CPU: a reply heard by several receivers of a shared decoder is published once.  The emulated
kernels (tests/sim/dedup_driver.cpp: adsb_dedup_device.h's four kernels inside the shared decoder's call, the host's rule for
the carry restated) against tests/golden/g_dedup.npz -- ONE unmodified reference decoder fed the publication sequence without
the duplicates (tools/make_golden_dedup.py) -- and against the plain-Python rule of tests/dedup_replay.py; the scan across
the wavefront, workgroup and LDS-tile seams; the carry's edges; the four kernels alone (sim_dedup_step) against a plain
statement of every output byte; the new translation unit's build facts.

What a green run here does NOT cover: the host's own branch of fleet_step, the entry points and their refusals, and
adsb_stream_reset beside the carry -- tests/test_gpu_dedup.py; and everything on the device's side of these seams: what hipcc
makes of k_dedup_find's LDS tiles and its __syncthreads() inside block-uniform loops, the real launchers' grid sizing (the
launches here are the driver's own) and the kernels' second grid-stride round under them, which needs more than 524 288
records -- tests/test_gpu_dedup_device.py runs this file's section "the kernels alone", unchanged, on the MI355X through
tests/gpu/dedup_device_driver.hip, and adds one step of 526 500 records built by period (periodic_step)."""
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
import test_mlat as TM
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


# ---- the kernels alone -----------------------------------------------------------------------------------------------------
# sim_dedup_step runs k_dedup_entries, _find, _merge and _mark on stated arrays, and every byte it returns has a plain statement
# here that never passes through the code under test: the entries are test_mlat.carry_words_numpy's words, dup[] is
# dedup_replay.find_duplicates', the merged buffer is NumPy's stable argsort over time_key, the cut is one float64 expression.
# The tests of this section (ALONE names them) use nothing of `sim` but sim_dedup_step: tests/test_gpu_dedup_device.py imports
# them unchanged and runs them on the device.  Each case first asserts, from the plain rule alone, that it reaches what it is
# meant to reach (Step.ranges: the three bounds k_dedup_find's workgroups share).
STATE_DTYPE = np.dtype([("off", "<i4"), ("cnt", "<i4"), ("hi", "<f8")])
W_DEMOD, W_LONG = np.uint64(N.BURST_DEMOD << 48), np.uint64(N.BURST_LONG << 48)
WG = 256                      # places per workgroup of k_dedup_find
GRIDS = (1, 3)


def words_of(ts, bits, mk, stream):
    if len(ts) == 0:
        return np.zeros((0, 4), np.uint64)
    return TM.carry_words_numpy(np.ascontiguousarray(ts, dtype=np.float64), np.ascontiguousarray(bits, dtype=np.uint8), np.asarray(mk, np.int32),
                                np.asarray(stream, np.int32))


def merge_and_cut(carry_words, ent, horizon):
    """-> (the merged buffer, the State): the stable merge of carry then call by time_key, hi the later of the two lists' last
    timestamps, off the count of entries with ts < hi - horizon in float64"""
    both = np.concatenate([carry_words, ent])
    merged = both[np.argsort(SR.time_key_np(both[:, 0].view(np.float64)), kind="stable")]
    ts = both[:, 0].view(np.float64)
    nc = len(carry_words)
    hi = ts[-1] if nc == 0 or ts[-1] >= ts[nc - 1] else ts[nc - 1]
    state = np.zeros(1, STATE_DTYPE)
    off = int((ts < hi - np.float64(horizon)).sum())
    state["off"], state["cnt"], state["hi"] = off, len(both) - off, hi
    return merged, state


def random_words(rng, shape):
    return rng.integers(0, 1 << 63, shape).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, shape).astype(np.uint64)


def records_of(rng, bits, dem, long_):
    """[n][4] record words: the PDU in words 2 and 3, ADSB_BURST_DEMOD and ADSB_BURST_LONG as stated, every other bit random"""
    n = len(bits)
    recs = random_words(rng, (n, 4))
    b16 = np.zeros((n, 16), np.uint8)
    b16[:, :14] = bits
    w = b16.view("<u8").reshape(n, 2)
    flags = recs[:, 3] & ~(np.uint64(0xFFFFFFFFFFFF) | W_DEMOD | W_LONG)
    recs[:, 2] = w[:, 0]
    recs[:, 3] = w[:, 1] | flags | np.where(dem, W_DEMOD, np.uint64(0)) | np.where(long_, W_LONG, np.uint64(0))
    return recs


class Step:
    """One sim_dedup_step: hearings (bits[m][14], ts[m], stream[m], dem[m], long[m]) of which those named by in_call are the
    call's list -- in the arrays' order, a stream's hearings contiguous -- and the others the carry, in time order.  Builds the
    entry's arguments and states every output."""

    def __init__(self, bits, ts, stream, in_call, window=0.002, horizon=1.0, dem=None, long_=None, extra_items=(), seed=1):
        rng = np.random.default_rng(seed)
        bits, ts, stream = np.asarray(bits, np.uint8), np.asarray(ts, np.float64), np.asarray(stream, np.int32)
        m = len(bits)
        dem = np.ones(m, bool) if dem is None else np.asarray(dem, bool)
        long_ = (bits[:, 0] >> 3) >= 16 if long_ is None else np.asarray(long_, bool)
        mk = np.where(dem, np.where(long_, 2, 1), 0).astype(np.int32)
        pay = [None if mk[i] == 0 else (112, bits[i].tobytes()) if mk[i] == 2 else (56, bits[i, :7].tobytes()) for i in range(m)]
        call = np.zeros(m, bool)
        call[in_call] = True
        ci, ki = np.flatnonzero(call), np.flatnonzero(~call)
        ki = ki[np.argsort(SR.time_key_np(ts[ki]), kind="stable")]
        self.window, self.horizon, self.n, self.nc = float(window), float(horizon), len(ci), len(ki)
        n = self.n
        assert n > 0
        # the carry
        self.carry_ts = ts[ki]
        self.carry = words_of(ts[ki], bits[ki], mk[ki], stream[ki])
        carry_list = [(float(ts[i]), pay[i], int(stream[i])) for i in ki]
        # the call's list, its items and its time order
        self.item_stream, self.first = call_list(stream[ci], n, extra_items)
        self.ts = ts[ci]
        self.exp_dup, order = DR.find_duplicates([pay[i] for i in ci], self.ts, stream[ci], carry_list, self.window)
        self.order = np.asarray(order, np.int32)
        assert np.array_equal(self.order, SR.time_order(self.ts))
        self.sorted_recs = records_of(rng, bits[ci], dem[ci], long_[ci])[self.order]
        self.sorted_ts = np.ascontiguousarray(self.ts[self.order])
        o = self.order
        self.exp_ent = words_of(self.sorted_ts, bits[ci][o], mk[ci][o], stream[ci][o])
        self.state_the_rest(rng)

    @classmethod
    def stated(cls, sorted_recs, sorted_ts, order, first, item_stream, carry, window, horizon, exp_ent, exp_dup, seed=1):
        """A step whose arguments, entries and dup[] the caller states (a case too large for __init__'s Python lists)"""
        self = cls.__new__(cls)
        self.window, self.horizon, self.n, self.nc = float(window), float(horizon), len(sorted_ts), len(carry)
        self.sorted_recs, self.sorted_ts, self.order = np.ascontiguousarray(sorted_recs), np.ascontiguousarray(sorted_ts), np.asarray(order, np.int32)
        self.first, self.item_stream = np.asarray(first, np.int32), np.asarray(item_stream, np.int32)
        self.carry, self.carry_ts = carry, carry[:, 0].copy().view(np.float64)
        self.exp_ent, self.exp_dup = exp_ent, np.asarray(exp_dup, np.int32)
        self.state_the_rest(np.random.default_rng(seed))
        return self

    def state_the_rest(self, rng):
        """from the arguments, the entries and dup[]: the time-ordered records behind k_dedup_find, the merged buffer and the
        cut, and delivered records and rows of random words with what k_dedup_mark must leave of them"""
        n, o = self.n, self.order
        self.exp_sorted = self.sorted_recs.copy()
        self.exp_sorted[self.exp_dup[o] != -1, 3] &= ~W_DEMOD
        self.exp_merged, self.exp_state = merge_and_cut(self.carry, self.exp_ent, self.horizon)
        self.recs, self.rows = random_words(rng, (n, 4)), random_words(rng, (n, 9))
        self.recs[:, 3] &= ~W_DEMOD                                      # as the decode step leaves a duplicate's: k_dedup_mark sets it
        marked = self.exp_dup != -1
        self.exp_recs, self.exp_rows = self.recs.copy(), self.rows.copy()
        self.exp_recs[marked, 3] |= W_DEMOD
        self.exp_rows[marked, 0] = (self.exp_rows[marked, 0] & ~np.uint64(0xFF)) | np.uint64(N.DEC_DUPLICATE)

    def place_of(self, t):
        """the place in the time order of list position t"""
        return int(np.flatnonzero(self.order == t)[0])

    def ranges(self, place):
        """(base, last, q_lo, c_lo, c_hi) of the workgroup that holds `place`, from the rule alone: q_lo the first place in
        front of base within the window of base's timestamp, [c_lo, c_hi) the carry entries that are neither in front of
        base's window nor behind last's."""
        base = place // WG * WG
        last = min(base + WG, self.n) - 1
        t0, t1 = self.sorted_ts[base], self.sorted_ts[last]
        near = np.flatnonzero(np.abs(t0 - self.sorted_ts[:base]) <= self.window)
        q_lo = int(near[0]) if len(near) else base
        c = self.carry_ts
        c_lo = int(((c < t0) & ~(np.abs(t0 - c) <= self.window)).sum())
        c_hi = int(((c <= t1) | (np.abs(t1 - c) <= self.window)).sum())
        return base, last, q_lo, c_lo, c_hi

    def carry_index(self, ts, stream):
        """the carry's entry with that timestamp and stream"""
        st = ((self.carry[:, 3] >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64)
        hit = np.flatnonzero((self.carry_ts == ts) & (st == stream))
        assert len(hit) == 1
        return int(hit[0])

    def run(self, sim, grid, rc=0):
        n, nc = self.n, self.nc
        out = dict(ent=np.zeros((n, 4), np.uint64), dup=np.zeros(n, np.int32), sorted=np.zeros((n, 4), np.uint64),
                   merged=np.zeros((nc + n, 4), np.uint64), state=np.zeros(1, STATE_DTYPE), recs=np.zeros((n, 4), np.uint64),
                   rows=np.zeros((n, 9), np.uint64))
        carry = np.ascontiguousarray(self.carry) if nc else np.zeros((1, 4), np.uint64)
        ins = [np.ascontiguousarray(x) for x in (self.sorted_recs, self.sorted_ts, self.order, self.first, self.item_stream, carry, self.recs,
                                                 self.rows)]
        p = [x.ctypes.data_as(vp) for x in ins]
        got = sim.sim_dedup_step(p[0], p[1], p[2], ctypes.c_int(n), p[3], p[4], ctypes.c_int(len(self.item_stream)), p[5], ctypes.c_int(nc),
                                 ctypes.c_double(self.window), ctypes.c_double(self.horizon), ctypes.c_int(grid), p[6], p[7],
                                 *[out[k].ctypes.data_as(vp) for k in ("ent", "dup", "sorted", "merged", "state", "recs", "rows")])
        assert got == rc, "guard or read-only input (-1), argument (-5), carry or cut (-6), a HIP status (<= -1000): %d" % got
        return out

    def check(self, sim, grids=GRIDS):
        """every output of the entry against its statement, as bytes, with each grid"""
        for grid in grids:
            got = self.run(sim, grid)
            assert got["ent"].tobytes() == self.exp_ent.tobytes(), ("entries", grid, np.flatnonzero((got["ent"] != self.exp_ent).any(1))[:5])
            bad = np.flatnonzero(got["dup"] != self.exp_dup)
            assert got["dup"].tobytes() == self.exp_dup.tobytes(), ("dup", grid, bad[:5], got["dup"][bad[:5]], self.exp_dup[bad[:5]])
            assert got["sorted"].tobytes() == self.exp_sorted.tobytes(), ("the time-ordered records", grid)
            assert got["merged"].tobytes() == self.exp_merged.tobytes(), ("merged", grid, np.flatnonzero((got["merged"] != self.exp_merged).any(1))[:5])
            assert got["state"].tobytes() == self.exp_state.tobytes(), ("state", grid, got["state"], self.exp_state)
            assert got["recs"].tobytes() == self.exp_recs.tobytes(), ("the marked records", grid)
            assert got["rows"].tobytes() == self.exp_rows.tobytes(), ("the marked rows", grid)
        return self


def ts_of(offset):
    """k_shared_keys' expression with every stream's start at T0"""
    return T0 + np.asarray(offset, np.int64).astype(np.float64) / FS


@pytest.mark.parametrize("n", [2, 65, 257, TILE + 1])
def test_alone_one_reply_heard_by_many_streams(sim, n):
    """In one call: the last hearing's workgroup stages every hearing in front of it.  With the first hearing in the carry:
    every hearing of the call is -2.  With n - 1 hearings in the carry and the earliest in time arriving last: the carry range
    is all of them, and all of them lie BEHIND the call's one record."""
    b, off, s = one_reply(n)
    w = Step(b, ts_of(off), s, np.arange(n))
    base, last, q_lo, _, _ = w.ranges(n - 1)
    assert last == n - 1 and q_lo == 0 and w.exp_dup[0] == -1 and (w.exp_dup[1:] == 0).all()
    w.check(sim)
    rev = np.arange(1, n)[::-1]                                        # the list in descending stream order: not the time order
    idx = np.concatenate([[0], rev])
    w = Step(b[idx], ts_of(off[idx]), s[idx], np.arange(1, n))
    assert (w.exp_dup == -2).all() and np.array_equal(w.order, np.arange(n - 1)[::-1]) and w.ranges(0)[3:] == (0, 1)
    w.check(sim)
    w = Step(b, ts_of(off), s, [0])
    assert w.exp_dup.tolist() == [-2] and w.ranges(0)[3:] == (0, n - 1) and (w.carry_ts > w.ts[0]).all()
    w.check(sim)


@pytest.mark.parametrize("front,between", [(TILE + 76, 5), (TILE + 300, 260), (2 * TILE + 9, 1)])
def test_alone_the_earliest_match_lies_in_a_later_partial_tile(sim, front, between):
    """seam_world in one call -- B's match A is staged at least one tile into the range, in the last, partial tile, and for
    (TILE + 300, 260) B's workgroup starts behind A -- and against the carry, where the same holds of the carry's range.  In
    both, the decoy on B's own stream lies in the first tile and must not count: where it is the only candidate, B is new."""
    b, off, s, (decoy, a, a2, bb) = seam_world(front, between)
    n = len(b)
    ts = ts_of(off)
    w = Step(b, ts, s, np.arange(n))
    base, last, q_lo, _, _ = w.ranges(w.place_of(bb))
    pa, pd = w.place_of(a), w.place_of(decoy)
    assert q_lo == 0 and pd - q_lo < TILE <= pa - q_lo and (pa - q_lo) // TILE == (last - 1 - q_lo) // TILE and (last - q_lo) % TILE != 0
    assert base > pa or (front, between) != (TILE + 300, 260)           # ... there B's workgroup starts behind A
    assert w.exp_dup[decoy] == -1 and w.exp_dup[a] == decoy and w.exp_dup[a2] == decoy and w.exp_dup[bb] == a
    w.check(sim)
    # against the carry: everything but B is there; the call is B and a hearing earlier than all of the carry
    hb, hts, hs = np.concatenate([b, [IDENT]]), np.concatenate([ts, ts_of([900])]), np.concatenate([s, [4]]).astype(np.int32)
    w = Step(hb, hts, hs, [bb, n])
    assert w.exp_dup.tolist() == [-2, -2]
    w.check(sim)
    # ... the carry's only hearing on another stream is A (A2 is on B's own now): found one tile into [c_lo, c_hi) or further
    s2 = s.copy()
    s2[a2] = 1
    w = Step(b, ts, s2, [bb])
    _, _, _, c_lo, c_hi = w.ranges(0)
    ia, idec = w.carry_index(ts[a], 0), w.carry_index(ts[decoy], 1)
    assert c_lo == 0 and c_hi == n - 1 and idec - c_lo < TILE <= ia - c_lo and (ia - c_lo) // TILE == (c_hi - 1 - c_lo) // TILE and (c_hi - c_lo) % TILE
    assert w.exp_dup.tolist() == [-2]
    w.check(sim)
    # ... and without A the decoy and A2, both on B's own stream, are all there is: B is new
    keep = np.delete(np.arange(n), a)
    w = Step(b[keep], ts[keep], s2[keep], [int(np.flatnonzero(keep == bb)[0])])
    assert w.exp_dup.tolist() == [-1] and w.nc == n - 2
    w.check(sim)
    # ... nor does the decoy count in the call
    keep = keep[np.argsort(s2[keep], kind="stable")]                   # the list: grouped by stream again
    w = Step(b[keep], ts[keep], s2[keep], np.arange(n - 1))
    assert (w.exp_dup == -1).all() and w.ranges(n - 2)[2] == 0
    w.check(sim)


def test_alone_more_than_two_tiles_of_hearings(sim):
    """2 * TILE + 10 hearings on stream 1, one on stream 0 behind them, forty more on stream 1: the forty's only match is staged
    more than two tiles into their workgroup's range."""
    k = 2 * TILE + 10
    n = k + 41
    who = np.ones(n, np.int32)
    who[k] = 0
    order = np.argsort(who, kind="stable")
    w = Step(np.tile(IDENT, (n, 1)), ts_of(1000 + np.arange(n))[order], who[order], np.arange(n))
    base, last, q_lo, _, _ = w.ranges(n - 1)
    assert q_lo == 0 and w.place_of(0) == k and k - q_lo >= 2 * TILE and last == n - 1
    assert w.exp_dup[0] == 1 and (w.exp_dup[1:k + 1] == -1).all() and (w.exp_dup[k + 1:] == 0).all()
    w.check(sim)


def test_alone_a_carry_range_on_both_sides_in_time(sim):
    """c_lo, c_hi and the carry's tile loop together: 300 records of the call (two workgroups) with a carry of 300 entries
    out of reach in front, 1200 within the window in front of the workgroup's first place, 1300 within it behind its last, and
    200 out of reach behind.  B (stream 1) lies in the second workgroup; its only match, A on stream 0, is among the late
    entries, in the range's last, partial tile; a decoy on stream 1 lies in the first.  A second reply is heard twice in the
    call, at places 100 and 290: the match lies in [q_lo, c_lo), so the call's tile loop must start at q_lo, not at c_lo."""
    early, front, back, late, n = 300, 1200, 1300, 200, 300
    off = np.concatenate([np.arange(early), 10000 - front + np.arange(front), 10000 + n + np.arange(back), 20000 + np.arange(late),
                          10000 + np.arange(n)])
    m = len(off)
    nc = m - n
    b = fillers(m, 77)
    s = np.full(m, 2, np.int32)
    i_decoy, i_a, i_b = early + 5, early + front + 1000, nc + 280
    for i, st_ in ((i_decoy, 1), (i_a, 0), (i_b, 1)):
        b[i], s[i] = IDENT, st_
    s[nc:i_b] = 3                                                      # the list: streams 3, 1, 2
    b[nc + 100] = b[nc + 290] = fillers(1, 5)[0]
    ts = ts_of(off)
    w = Step(b, ts, s, np.arange(nc, m))
    place = w.place_of(280)
    base, last, q_lo, c_lo, c_hi = w.ranges(place)
    assert (base, last) == (WG, n - 1) and place == 280
    c = w.carry_ts
    assert c_lo == early and c_hi == nc - late and ((c[c_lo:c_hi] < w.sorted_ts[base]).sum(), (c[c_lo:c_hi] > w.sorted_ts[last]).sum()) == (front, back)
    assert front > TILE and back > TILE
    ia, idec = w.carry_index(ts[i_a], 0), w.carry_index(ts[i_decoy], 1)
    assert idec - c_lo < TILE and (ia - c_lo) // TILE == (c_hi - 1 - c_lo) // TILE == 2 and (c_hi - c_lo) % TILE != 0
    assert w.ranges(0)[3:] == (early, nc - late) and (w.exp_dup != -1).sum() == 2 and w.exp_dup[280] == -2
    assert w.exp_dup[290] == 100 and q_lo <= 100 < c_lo and s[nc + 100] != s[nc + 290]
    w.check(sim)
    # the same carry without A: nothing matches
    keep = np.delete(np.arange(m), i_a)
    w = Step(b[keep], ts[keep], s[keep], np.arange(nc - 1, m - 1))
    assert np.flatnonzero(w.exp_dup != -1).tolist() == [290]
    w.check(sim)


def test_alone_all_timestamps_equal(sim):
    """Bit-equal timestamps, 300 in the call and 300 in the carry, window 0.002 and window 0: the list order is the time order,
    and on equal keys the merge puts the carry first."""
    n = 300
    b, _, s = one_reply(2 * n)
    ts = np.full(2 * n, T0 + 5000 / FS)
    for window in (0.002, 0.0):
        w = Step(b[:n], ts[:n], s[:n], np.arange(n), window=window)
        assert np.array_equal(w.order, np.arange(n)) and w.exp_dup[0] == -1 and (w.exp_dup[1:] == 0).all() and w.ranges(n - 1)[2] == 0
        w.check(sim)
        w = Step(b, ts, s, np.arange(n, 2 * n), window=window)
        assert (w.exp_dup == -2).all() and w.ranges(n - 1)[3:] == (0, n)
        assert w.exp_merged.tobytes() == np.concatenate([w.carry, w.exp_ent]).tobytes()
        w.check(sim)


def test_alone_window_zero(sim):
    """window = 0: one sample apart is another transmission, in the call and against the carry."""
    b, _, s = one_reply(6)
    off = np.array([5000, 5000, 5001, 5001, 5001, 5002])
    w = Step(b[:4], ts_of(off[:4]), s[:4], np.arange(4), window=0.0)
    assert w.exp_dup.tolist() == [-1, 0, -1, 2]
    w.check(sim)
    w = Step(b, ts_of(off), s, [4, 5], window=0.0)                     # stream 4 at 5001: streams 2 and 3 were there; stream 5 at 5002: nobody
    assert w.exp_dup.tolist() == [-2, -1] and w.ranges(0)[3:] == (2, 4)
    w.check(sim)


def test_alone_records_with_marker_zero(sim):
    """A record without ADSB_BURST_DEMOD takes no part: in the call it is no match and no duplicate, in the carry it is no
    match, and a call where nobody takes part marks nothing and still merges and moves hi."""
    b, off, s = one_reply(6)
    ts = ts_of(off)
    w = Step(b, ts, s, np.arange(6), dem=[0, 1, 0, 1, 1, 0])
    assert w.exp_dup.tolist() == [-1, -1, -1, 1, 1, -1] and (w.exp_ent[[0, 2, 5], 3] >> np.uint64(56) == 0).all()
    assert not w.exp_ent[[0, 2, 5], 1:3].any()
    w.check(sim)
    w = Step(b, ts, s, [3, 4, 5], dem=[0, 0, 0, 1, 1, 1])
    assert w.exp_dup.tolist() == [-1, 0, 0] and w.ranges(0)[3:] == (0, 3)
    w.check(sim)
    w = Step(b, ts, s, [3, 4, 5], dem=[1, 1, 1, 0, 0, 0])
    assert (w.exp_dup == -1).all() and w.exp_state["hi"][0] == ts[5] and w.exp_state["cnt"][0] == 6
    w.check(sim)
    # short and long with the same first 56 bits, and a short reply's bytes 7 .. 13, which are not payload
    b2 = np.tile(IDENT, (4, 1))
    b2[1, 7:] ^= 0xFF
    w = Step(b2, ts[:4], s[:4], np.arange(4), long_=[0, 0, 1, 1])
    assert w.exp_dup.tolist() == [-1, 0, -1, 2]
    w.check(sim)


def test_alone_the_merge_and_the_cut(sim):
    """k_dedup_merge's edges.  Ties on both sides (the carry first); nc = 0; n = 1; a call wholly behind hi - horizon; an entry
    at exactly hi - horizon is kept and the double below it is dropped; hi from the carry."""
    b, _, s = one_reply(12)
    # ties on both sides: the carry and the call both hold several entries at 4000 and at 6000
    off = np.array([4000, 6000, 4000, 6000, 6000, 4000, 4000, 6000, 5000, 4000, 6000, 6000])
    w = Step(b, ts_of(off), s, np.arange(6, 12))
    st = ((w.exp_merged[:, 3] >> np.uint64(32)) & np.uint64(0xFFFFFF)).tolist()
    assert st == [0, 2, 5, 6, 9, 8, 1, 3, 4, 7, 10, 11]              # per timestamp: the carry's in its order, then the call's in list order
    w.check(sim)
    # nc = 0, and n = 1 with and without a carry
    w = Step(b[:5], ts_of(off[:5]), s[:5], np.arange(5))
    assert w.nc == 0 and w.exp_state.tolist() == [(0, 5, T0 + 6000 / FS)]
    w.check(sim)
    Step(b[:1], ts_of(off[:1]), s[:1], [0]).check(sim)
    Step(b[:6], ts_of(off[:6]), s[:6], [2]).check(sim)
    # the cut, horizon 1: hi = T0 + 3 is the call's last; T0 + 2 is kept, the double below it is not
    edge = T0 + 2.0
    ts = np.array([T0, np.nextafter(edge, -np.inf), edge, T0 + 2.5, T0 + 0.5, np.nextafter(edge, -np.inf), edge, T0 + 3.0])
    w = Step(b[:8], ts, s[:8], np.arange(4, 8))
    assert T0 + 3.0 - 1.0 == edge and w.exp_state.tolist() == [(4, 4, T0 + 3.0)]
    assert (w.exp_merged[:4, 0].view(np.float64) < edge).all() and (w.exp_merged[4:, 0].view(np.float64) >= edge).all()
    w.check(sim)
    # a call wholly behind hi - horizon, hi the carry's: the cut takes all of it and the old carry's head
    ts = np.array([T0 + 1.5, T0 + 2.5, T0 + 4.0, T0 + 1.0, T0 + 2.0, T0 + 2.0 + 1 / FS])
    w = Step(b[:6], ts, s[:6], [3, 4, 5])
    assert w.exp_state.tolist() == [(5, 1, T0 + 4.0)] and w.exp_dup.tolist() == [-1, -1, 1]
    w.check(sim)
    # hi from the carry, the call inside the horizon; and the two last timestamps equal
    ts = np.array([T0 + 1.5, T0 + 4.0, T0 + 3.5, T0 + 3.75])
    w = Step(b[:4], ts, s[:4], [2, 3])
    assert w.exp_state.tolist() == [(1, 3, T0 + 4.0)]
    w.check(sim)
    ts = np.array([T0 + 1.5, T0 + 4.0, T0 + 3.5, T0 + 4.0])
    w = Step(b[:4], ts, s[:4], [2, 3], window=0.0)
    assert w.exp_state.tolist() == [(1, 3, T0 + 4.0)] and w.exp_dup.tolist() == [-1, -2]
    w.check(sim)


def test_alone_items(sim):
    """first[] with an empty first, an empty middle and an empty last item, and all three; stream numbers 0 and 0xFFFFFF."""
    b, off, _ = one_reply(9)
    s = np.array([0, 0, 0, 0xFFFFFF, 0xFFFFFF, 7, 7, 7, 7], np.int32)
    ts = ts_of(off[::-1])                                              # the time order is the list reversed
    for extra, first in ((((0, 11),), [0, 0, 3, 5, 9]), (((1, 11),), [0, 3, 3, 5, 9]), (((3, 11),), [0, 3, 5, 9, 9]),
                         (((0, 11), (2, 12), (5, 13)), [0, 0, 3, 3, 5, 9, 9])):
        w = Step(b, ts, s, np.arange(9), extra_items=extra)
        assert w.first.tolist() == first
        got = ((w.exp_ent[:, 3] >> np.uint64(32)) & np.uint64(0xFFFFFF)).tolist()
        assert got == s[::-1].tolist() and w.exp_dup.tolist() == [8, 8, 8, 8, 8, -1, -1, -1, -1]
        w.check(sim)
    # the first record of the carry is stream 0xFFFFFF's; stream 0 hears it again
    w = Step(b[:2], ts_of([1000, 1001]), np.array([0xFFFFFF, 0], np.int32), [1], extra_items=((0, 5), (2, 6)))
    assert w.exp_dup.tolist() == [-2] and w.first.tolist() == [0, 0, 1, 1]
    w.check(sim)


# One step built by period, as test_mlat.periodic builds its carry: P_PERIOD = 65 records of the call (coprime to 64, 256 and
# 1024: every hearing drifts over every lane, workgroup place and tile place), all within the window, repeated every
# P_SPACING = 2^-5 s -- sixteen windows -- from P_EPOCH = 1024 s on.  Every P_CARRY_EVERY-th period also has 65 entries of the
# carry, interleaved in time with the call's.  Every timestamp is a multiple of 2^-21 s below 2048 s, so the shift is exact and
# period k's verdicts are period 0's (or, beside the carry, period 0's against period 0's carry), shifted; those two come
# from find_duplicates.
P_EPOCH, P_SPACING, P_TICK, P_PERIOD, P_WINDOW, P_CARRY_EVERY = 1024.0, 2.0 ** -5, 2.0 ** -21, 65, 2.0 ** -9, 127


def period0():
    """-> (the call's (tick, bits, stream, marker) in time order, ties in stream order, and the carry's): a long reply heard by
    streams 0 .. 4 (the carry: by stream 6); a short one heard by streams 5, 6 and 5 again (the carry: by 5); a marker-0
    record with the long reply's bytes; a reply heard by streams 2 and 6 at the same tick; fillers on all eight streams."""
    short = IDENT.copy()
    short[0] = 0x5D                                                    # DF 11
    call = [(6 + 10 * s_, IDENT, s_, 2) for s_ in range(5)] + [(60, short, 5, 1), (64, short, 6, 1), (90, short, 5, 1), (30, IDENT, 7, 0)]
    other = fillers(1, 3)[0]
    call += [(100, other, 2, 2), (100, other, 6, 2)]
    fb = fillers(2 * P_PERIOD, 9)
    call += [(200 + 14 * k, fb[k], k % 8, 2) for k in range(P_PERIOD - len(call))]
    carry = [(21, IDENT, 6, 2), (71, short, 5, 1)]
    carry += [(201 + 14 * k, fb[P_PERIOD + k], (k + 3) % 8, 2 if k % 5 else 0) for k in range(P_PERIOD - len(carry))]
    out = []
    for rows in (call, carry):
        rows = sorted(rows, key=lambda r: (r[0], r[2]))
        assert len(rows) == P_PERIOD and len(set((r[0], r[2]) for r in rows)) == P_PERIOD
        out.append((np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.uint8), np.array([r[2] for r in rows], np.int32),
                    np.array([r[3] for r in rows], np.int32)))
    return out


def periodic_step(periods, horizon, seed=3):
    """-> (Step, period 0's dup[] without and beside the carry, as places within the period)"""
    (tick, bits, stream, mk), (ctick, cbits, cstream, cmk) = period0()
    assert max(tick.max(), ctick.max()) * P_TICK < P_WINDOW < P_SPACING / 8 and np.gcd(P_PERIOD, 64 * 256 * 1024) == 1
    pay = lambda b, m: [None if m[i] == 0 else (112, b[i].tobytes()) if m[i] == 2 else (56, b[i, :7].tobytes()) for i in range(len(b))]      # noqa: E731
    t0, c0 = P_EPOCH + tick * P_TICK, P_EPOCH + ctick * P_TICK
    d_alone, o1 = DR.find_duplicates(pay(bits, mk), t0, stream, [], P_WINDOW)
    d_carry, o2 = DR.find_duplicates(pay(bits, mk), t0, stream, list(zip(c0.tolist(), pay(cbits, cmk), cstream.tolist())), P_WINDOW)
    assert np.array_equal(o1, np.arange(P_PERIOD)) and np.array_equal(o2, o1)      # given in time order: a list position is a place
    assert sorted(set(d_alone.tolist())) != sorted(set(d_carry.tolist())) and (d_carry == -2).sum() >= 6 and (d_alone >= 0).sum() >= 7
    ks = np.arange(periods)
    with_carry = ks % P_CARRY_EVERY == 0
    n = periods * P_PERIOD
    ts = (P_EPOCH + ks[:, None] * P_SPACING + tick[None, :] * P_TICK).ravel()
    assert ts[-1] < 2 * P_EPOCH and ((ts.reshape(periods, P_PERIOD) - ks[:, None] * P_SPACING) == t0[None, :]).all()      # the shift is exact
    cts = (P_EPOCH + ks[with_carry][:, None] * P_SPACING + ctick[None, :] * P_TICK).ravel()
    kc = int(with_carry.sum())
    carry = words_of(cts, np.tile(cbits, (kc, 1)), np.tile(cmk, kc), np.tile(cstream, kc))
    s_all, mk_all, bits_all = np.tile(stream, periods), np.tile(mk, periods), np.tile(bits, (periods, 1))
    lst = np.argsort(s_all, kind="stable")                             # the list, grouped by stream: list position -> place
    order = np.empty(n, np.int32)
    order[lst] = np.arange(n, dtype=np.int32)                          # place -> list position
    assert (np.diff(ts) >= 0).all()
    assert np.array_equal(np.lexsort((order, ts)), np.arange(n))       # ascending (ts, list position) is the place order
    counts = np.bincount(s_all, minlength=8)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    first, item_stream = np.insert(first, 3, first[3]), np.insert(np.arange(8, dtype=np.int32), 3, 0xABCDEF)      # and an empty item
    d = np.where(with_carry[:, None], d_carry[None, :], d_alone[None, :])
    place = np.where(d >= 0, d + ks[:, None] * P_PERIOD, 0).ravel()
    d = d.ravel()
    dup = np.empty(n, np.int32)
    dup[order] = np.where(d >= 0, order[place], d)
    rng = np.random.default_rng(seed)
    w = Step.stated(records_of(rng, bits_all, mk_all != 0, mk_all == 2), ts, order, first, item_stream, carry, P_WINDOW, horizon,
                    words_of(ts, bits_all, mk_all, s_all), dup, seed)
    return w, d_alone, d_carry


def test_a_step_built_by_period(sim):
    """The builder of tests/test_gpu_dedup_device.py's large case at 300 periods (19 500 records, three periods beside the
    carry), on the emulator: period 0 alone through Step's own statement gives the same bytes as the builder's."""
    w, d_alone, d_carry = periodic_step(300, 4.0)
    assert w.n == 300 * P_PERIOD and w.nc == 3 * P_PERIOD and 0 < w.exp_state["off"][0] < w.n
    w.check(sim, grids=(3,))
    (tick, bits, stream, mk), (ctick, cbits, cstream, cmk) = period0()
    lst = np.argsort(stream, kind="stable")
    one = Step(np.concatenate([bits[lst], cbits]), P_EPOCH + np.concatenate([tick[lst], ctick]) * P_TICK, np.concatenate([stream[lst], cstream]),
               np.arange(P_PERIOD), window=P_WINDOW, horizon=4.0, dem=np.concatenate([mk[lst], cmk]) != 0,
               long_=np.concatenate([mk[lst], cmk]) == 2)
    assert np.array_equal(np.where(d_carry >= 0, one.order[np.maximum(d_carry, 0)], d_carry), one.exp_dup[one.order])
    one.check(sim, grids=(1,))


ALONE = ("test_alone_one_reply_heard_by_many_streams", "test_alone_the_earliest_match_lies_in_a_later_partial_tile",
         "test_alone_more_than_two_tiles_of_hearings", "test_alone_a_carry_range_on_both_sides_in_time", "test_alone_all_timestamps_equal",
         "test_alone_window_zero", "test_alone_records_with_marker_zero", "test_alone_the_merge_and_the_cut", "test_alone_items")


def test_alone_names_the_section():
    """ALONE is what tests/test_gpu_dedup_device.py imports: every test of this section, and nothing else"""
    assert sorted(ALONE) == sorted(k for k in globals() if k.startswith("test_alone_") and k != "test_alone_names_the_section")


def test_the_step_entry_refuses_bad_arguments(sim):
    """-5: an order that is no permutation, a first[] that does not end at n or goes down, a negative size."""
    b, off, s = one_reply(4)
    w = Step(b, ts_of(off), s, np.arange(4))

    def rc_of(**change):
        v = Step(b, ts_of(off), s, np.arange(4))
        for k, x in change.items():
            setattr(v, k, np.asarray(x, getattr(v, k).dtype))
        v.run(sim, 1, rc=-5)
    rc_of(order=[0, 1, 1, 3])
    rc_of(order=[0, 1, 2, 4])
    rc_of(first=[0, 1, 2, 3, 5])
    rc_of(first=[0, 2, 1, 3, 4])
    rc_of(first=[1, 1, 2, 3, 4])
    w.check(sim, grids=(2,))


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
