"""The fleet's merged picture on the CPU (adsb_stream_planes_merged: one row per aircraft out of every receiver's
plane_dict): the emulated kernels (tests/sim/merge_driver.cpp: k_merge_keys, the library's radix sort, k_merge_heads, its
scan, k_merge_emit, over the store the emulated fleet step builds) against tests/golden/g_merge.npz -- one UNMODIFIED
reference decoder per stream and the table tools/make_golden_merge.py folds their plane_dicts into -- and against a
plain-Python fold over test_expire.FleetModel's per-stream dicts, itself checked against the golden's table first; the Python
layer (_native.Context.merged_planes, frontend.Receivers.merged / .table); the declared symbol and the kernels' resources.

The expected value is never the code under test.  What a green run here does NOT cover: the driver restates the host's
argument rules and launch order (adsb_hip.hip adsb_stream_planes_merged); the host code itself runs in
tests/test_gpu_merge.py only.

A cutoff hides entries from the old end (last_seen < cutoff), so it can never hide an aircraft's freshest entry and keep an
older one; the case the golden holds instead: the cutoff hides the OLDER entry that alone had a group, the group goes
(src -1) and the fresher entry keeps the aircraft."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import decode_streams as S
import test_decode as TD
import test_expire as TE
import test_planes as TP
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
MERGE_SO = os.path.join(SIM_DIR, "libadsb_merge_sim.so")
GOLD = os.path.join(HERE, "golden", "g_merge.npz")
PARENT_KERNELS = os.path.join(HERE, "golden", "merge_parent_kernels.json")
CONFIGS = TE.CONFIGS
INT64_MIN = -(1 << 63)
NAN = float("nan")
vp = ctypes.c_void_p
SRC = ("src_callsign", "src_altitude", "src_velocity", "src_position")


def merge_lib():
    srcs = [os.path.join(SIM_DIR, f) for f in ("merge_driver.cpp", "expire_driver.cpp", "planes_driver.cpp", "fleet_driver.cpp",
                                               "decode_driver.cpp", "sim_support.h", "hipsim.h")] + \
        [os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not (os.path.exists(MERGE_SO) and all(os.path.getmtime(MERGE_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", MERGE_SO])
    lib = ctypes.CDLL(MERGE_SO)
    lib.sim_exp_fleet_open.restype = ctypes.c_void_p
    lib.sim_exp_fleet_slot_of.restype = ctypes.c_longlong
    lib.sim_exp_fleet_home.restype = ctypes.c_uint
    lib.sim_fleet_taken.restype = ctypes.c_longlong
    lib.sim_fleet_gen_max.restype = ctypes.c_uint
    lib.sim_fleet_get_call.restype = ctypes.c_ulonglong
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = merge_lib()
    assert lib.sim_merge_info_bytes() == N.MERGED_DTYPE.itemsize == 32
    assert lib.sim_dec_row_bytes() == N.DECODED_DTYPE.itemsize and lib.sim_fleet_slot_bytes() == 104
    return lib


@pytest.fixture(scope="module")
def gm():
    return np.load(GOLD)


def constants(lib):
    v = [ctypes.c_int() for _ in range(5)]
    lib.sim_merge_constants(*[ctypes.byref(x) for x in v])
    return dict(zip(("chunk", "threads", "tile", "stream_bits", "addr_bits"), (x.value for x in v)))


class MergedFleet(TE.AgedFleet):
    """test_expire.AgedFleet with the merged picture (merge_driver.cpp's sim_merge_fleet over the same handle)."""

    def merged_rc(self, streams=None, cutoff=INT64_MIN, grid=3, cap=None, rows=True, info=True, keys=None):
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        k = 0 if sel is None else len(sel)
        cap = self.stats()["planes"] if cap is None else cap
        r, f = np.zeros(cap, dtype=N.DECODED_DTYPE), np.zeros(cap, dtype=N.MERGED_DTYPE)
        r.view(np.uint8)[:] = 0x77
        f.view(np.uint8)[:] = 0x77
        n, nk = ctypes.c_int(-1), ctypes.c_int(-1)
        sp = None if sel is None else (sel.ctypes.data_as(vp) if k else ctypes.cast(ctypes.byref(n), vp))
        rc = self.lib.sim_merge_fleet(self.h, sp, ctypes.c_int(k), ctypes.c_longlong(cutoff), ctypes.c_int(grid), ctypes.c_int(cap),
                                      r.ctypes.data_as(vp) if rows and cap else None, f.ctypes.data_as(vp) if info and cap else None,
                                      ctypes.byref(n), None if keys is None else keys.ctypes.data_as(vp), ctypes.byref(nk))
        return rc, r, f, n.value, nk.value

    def merged(self, streams=None, cutoff=INT64_MIN, **kw):
        rc, r, f, n, _ = self.merged_rc(streams, cutoff, **kw)
        assert rc == 0, rc
        return r[:n], f[:n]


# ---- the expectation: a plain fold over per-stream dicts -----------------------------------------------------------------------
def fold(models, sel, cutoff=INT64_MIN):
    """models[s]: test_expire.Model (decode_replay's plane entries and last_seen); sel: stream indices, ascending -> (rows, info)
    by the header's rule: contributing = selected and last_seen >= cutoff; num_msgs the sum modulo 2^32; each group from the
    contributing entry that has it and has the greatest last_seen, the lowest stream among equals."""
    has = (lambda p: p["callsign"] is not None, lambda p: p["altitude"] is not None, lambda p: p["vel"] is not None,
           lambda p: not np.isnan(p["lat"]))
    groups = (("callsign",), ("altitude",), ("vel",), ("lat", "lon"))
    table = {}
    for s in sel:
        for a, p in models[s].d.planes.items():
            t = models[s].seen[a]
            if t < cutoff:
                continue
            m = table.setdefault(a, dict(p=dict(callsign=None, altitude=None, vel=None, lat=NAN, lon=NAN, n=0), seen=t, n=0,
                                         src=[-1] * 4, t=[None] * 4))
            m["n"] += 1
            m["seen"] = max(m["seen"], t)
            m["p"]["n"] = (m["p"]["n"] + p["n"]) % (1 << 32)
            for g in range(4):
                if has[g](p) and (m["src"][g] < 0 or t > m["t"][g]):
                    for k in groups[g]:
                        m["p"][k] = p[k]
                    m["src"][g], m["t"][g] = s, t
    rows = TP.plane_rows({a: m["p"] for a, m in table.items()})
    info = np.zeros(len(table), dtype=N.MERGED_DTYPE)
    for i, a in enumerate(sorted(table)):
        m = table[a]
        info[i] = (m["seen"], m["n"]) + tuple(m["src"]) + (0,)
    return rows, info


def same(got, exp, what=""):
    """(rows, info) byte for byte"""
    TP.rows_equal(got[0], exp[0])
    assert got[1].dtype == exp[1].dtype == N.MERGED_DTYPE and got[1].tobytes() == exp[1].tobytes(), (what, got[1], exp[1])


# ---- the golden ----------------------------------------------------------------------------------------------------------------
ENTRY = ("icao", "cs", "csset", "alt", "altset", "speed", "heading", "vrate", "vrset", "lat", "lon", "nmsgs")


def gold_case(gm, tag, case):
    m = np.flatnonzero(gm["m_case_" + tag] == case)
    e = {k: gm["m_%s_%s" % (k, tag)][m] for k in ENTRY}
    info = np.zeros(len(m), dtype=N.MERGED_DTYPE)
    info["last_seen"], info["n_streams"] = gm["m_seen_" + tag][m], gm["m_nstreams_" + tag][m]
    for g, name in enumerate(SRC):
        info[name] = gm["m_src_" + tag][m, g]
    return e, info


def cases(gm):
    """[(case number, selection or None, cutoff)]"""
    n = int(gm["n_streams"])
    sels = [None if len(gm["sel_%d" % i]) == 0 else [int(x) for x in gm["sel_%d" % i]] for i in range(2)]
    assert sels[0] is None and all(0 <= x < n for x in sels[1])
    return [(2 * si + ci, sels[si], int(gm["cutoffs"][ci])) for si in range(2) for ci in range(2)]


def check_case(got, gm, tag, case):
    e, info = gold_case(gm, tag, case)
    TP.check_against_golden(got[0], e, (tag, case))
    assert got[1].tobytes() == info.tobytes(), (tag, case, got[1], info)


def row_of(gm, tag, case, addr):
    e, info = gold_case(gm, tag, case)
    i = np.flatnonzero(e["icao"] == addr)
    return None if len(i) == 0 else ({k: v[i[0]] for k, v in e.items()}, info[i[0]])


def test_golden_holds_the_cases(gm):
    """What tools/make_golden_merge.py promises, read from the file alone."""
    W, X, Y, Z = 0x4B1A01, 0x3C65A2, 0xA0F003, 0x71BC04
    assert int(gm["n_streams"]) == 5 and gm["cutoffs"][0] == INT64_MIN and len(gm["bits"]) == len(gm["ts"]) == len(gm["stream"])
    for tag, filt, corr in CONFIGS:
        blanks = np.bincount(gm["f_stream_" + tag][gm["f_icao_" + tag] < 0], minlength=5)
        assert blanks.max() <= (1 if corr == "Conservative" else 0), (tag, blanks)
        # every group from another stream
        e, f = row_of(gm, tag, 0, W)
        assert sorted(int(f[k]) for k in SRC) == [0, 1, 2, 3] and f["n_streams"] == 4, (tag, f)
        assert e["csset"] and e["altset"] and e["vrset"] and e["lat"] != TD.NAN_BITS
        # a last_seen tie between two streams: the lower one's callsign
        e, f = row_of(gm, tag, 0, X)
        seen = {int(s): int(t) for s, a, t in zip(gm["f_stream_" + tag], gm["f_icao_" + tag], gm["f_seen_" + tag]) if a == X}
        cs = {int(s): bytes(c) for s, a, c in zip(gm["f_stream_" + tag], gm["f_icao_" + tag], gm["f_cs_" + tag]) if a == X}
        assert sorted(seen) == [1, 2] and seen[1] == seen[2] and cs[1] != cs[2]
        assert f["src_callsign"] == 1 and bytes(e["cs"]) == cs[1] and f["src_velocity"] == 2
        # a group only the oldest entry has
        e, f = row_of(gm, tag, 0, Y)
        seen = {int(s): int(t) for s, a, t in zip(gm["f_stream_" + tag], gm["f_icao_" + tag], gm["f_seen_" + tag]) if a == Y}
        assert f["src_velocity"] == min(seen, key=seen.get) and f["src_callsign"] == max(seen, key=seen.get) and len(seen) == 3
        # the cutoff hides the entry that held a group: the group goes, a fresher entry keeps the aircraft
        (e0, f0), (e1, f1) = row_of(gm, tag, 0, Z), row_of(gm, tag, 1, Z)
        assert f0["n_streams"] == 2 and f0["src_velocity"] == 0 and e0["vrset"] == 1
        assert f1["n_streams"] == 1 and f1["src_velocity"] == -1 and e1["vrset"] == 0 and f1["src_callsign"] == 3
        assert e1["nmsgs"] < e0["nmsgs"]
        # the cutoff hides an aircraft of exactly one stream entirely; both ends of the address space
        e, f = row_of(gm, tag, 0, 0x000000)
        assert f["n_streams"] == 1 and row_of(gm, tag, 1, 0x000000) is None
        assert row_of(gm, tag, 0, 0xFFFFFF)[1]["n_streams"] == 2 and row_of(gm, tag, 1, 0xFFFFFF)[1]["n_streams"] == 1
        # the selection matters
        assert row_of(gm, tag, 2, W)[1]["n_streams"] == 2 and row_of(gm, tag, 2, 0x000000) is None


def streams_of(gm):
    return gm["bits"], gm["ts"], gm["stream"]


def gold_models(gm, filt, corr):
    mod = TE.FleetModel(int(gm["n_streams"]), filt, corr)
    mod.call(*streams_of(gm))
    return mod


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_model_fold_equals_golden(gm, tag, filt, corr):
    """The test's own fold, over the model's per-stream dicts, gives the table the tool folded from the reference's; the
    per-stream dicts are the reference's too."""
    mod = gold_models(gm, filt, corr)
    for s, m in enumerate(mod.m):
        rows, seen = m.snapshot()
        keep = np.flatnonzero((gm["f_stream_" + tag] == s) & (gm["f_icao_" + tag] >= 0))
        keep = keep[np.argsort(gm["f_icao_" + tag][keep], kind="stable")]
        TP.check_against_golden(rows, {k: gm["f_%s_%s" % (k, tag)][keep] for k in ENTRY}, (tag, s))
        assert np.array_equal(seen, gm["f_seen_" + tag][keep])
    for case, sel, cutoff in cases(gm):
        check_case(fold(mod.m, range(len(mod.m)) if sel is None else sel, cutoff), gm, tag, case)


@pytest.mark.parametrize("chunk", (1000, 4))
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_emulated_fleet_equals_golden(sim, gm, tag, filt, corr, chunk):
    """The golden's PDU lists through the emulated fleet step, all at once and four PDUs a call; every stored selection and
    cutoff through the emulated k_merge_*: rows and info byte-equal to the stored table."""
    f = MergedFleet(sim, int(gm["n_streams"]), filt, corr)
    b, t, s = streams_of(gm)
    for lo in range(0, len(b), chunk):
        f.call(b[lo:lo + chunk], t[lo:lo + chunk], s[lo:lo + chunk])
    for case, sel, cutoff in cases(gm):
        for grid in (1, 3):
            check_case(f.merged(sel, cutoff, grid=grid), gm, tag, case)
    f.close()


# ---- fleets built here ---------------------------------------------------------------------------------------------------------
def velocity(aa, rng):
    body = rng.integers(0, 2, 51).astype(np.uint8)
    body[:3] = S.ib(1, 3)
    return np.packbits(S.es(aa, 19, body))


def position(aa, odd, lat, lon, rng):
    la, lo = S.cpr_encode(lat, lon, odd)
    body = np.zeros(51, np.uint8)
    body[3:15], body[16], body[17:34], body[34:51] = S.ib(int(rng.integers(0, 4096)), 12), odd, S.ib(la, 17), S.ib(lo, 17)
    return np.packbits(S.es(aa, 11, body))


def traffic(pairs, rng, t0=5000.5, spread=6):
    """One to three replies for every (stream, address): an identification, a velocity, one position frame (an altitude) or a
    pair of them (a fix), at whole seconds out of a handful, so that last_seen ties are common -> bits, ts, streams."""
    b, t, s = [], [], []
    for stream, a in pairs:
        kind = int(rng.integers(0, 5))
        at = t0 + int(rng.integers(0, spread))
        if kind == 0:
            new = [TE.ident(a, rng)]
        elif kind == 1:
            new = [velocity(a, rng)]
        elif kind == 2:
            new = [position(a, int(rng.integers(0, 2)), 40.0, 5.0, rng)]
        elif kind == 3:
            lat, lon = float(rng.uniform(-60, 60)), float(rng.uniform(-170, 170))
            new = [position(a, 0, lat, lon, rng), position(a, 1, lat, lon, rng)]
        else:
            new = [TE.ident(a, rng), velocity(a, rng)]
        for k, x in enumerate(new):
            b.append(x); t.append(at + 0.25 * k); s.append(stream)
    return np.array(b, np.uint8), np.array(t, np.float64), np.array(s, np.int32)


class Models(dict):
    """stream -> test_expire.Model, made on first use (a fleet of thousands of streams with a handful in use)"""

    def __init__(self, filt="All Messages", corr="None"):
        dict.__init__(self)
        self.cfg = (filt, corr)

    def __missing__(self, s):
        self[s] = TE.Model(*self.cfg)
        return self[s]

    def call(self, b, t, s):
        for x, y, k in zip(b, t, s):
            self[int(k)].row(x, y)


def feed(f, mod, pairs, rng, **kw):
    b, t, s = traffic(pairs, rng, **kw)
    f.call(b, t, s)
    mod.call(b, t, s)


def test_segments_across_every_seam(sim):
    """70 streams x 60 shared aircraft and 22 aircraft of one stream each: 4222 sorted keys, more than one sort tile.  One
    aircraft's segment lies across sorted rows 63 / 64 (two head counts), another across 255 / 256 (two workgroups), another
    across 4095 / 4096 (two sort tiles); one head is a workgroup's last row and the next head the following workgroup's first.
    The placements are asserted from the key arithmetic."""
    c = constants(sim)
    assert c == dict(chunk=64, threads=256, tile=4096, stream_bits=20, addr_bits=24)
    rng = np.random.default_rng(81)
    n_streams, shared = 70, [0x100000 + 64 * i for i in range(60)]
    pads = [(int(7 * k % n_streams), shared[6] + 1 + k) for k in range(22)]
    pairs = [(s, a) for a in shared for s in range(n_streams)] + pads
    keys = np.array(sorted((a << c["stream_bits"]) | s for s, a in pairs), np.uint64)
    addr = keys >> np.uint64(c["stream_bits"])
    head = np.concatenate([[True], addr[1:] != addr[:-1]])
    assert len(keys) == 4222 > c["tile"]
    for seam in (c["chunk"], c["threads"], c["tile"]):
        assert addr[seam - 1] == addr[seam] and not head[seam], seam                      # a segment lies across it
    edge = [j for j in range(c["threads"] - 1, len(keys) - 1, c["threads"]) if head[j] and head[j + 1]]
    assert edge == [2 * c["threads"] - 1]                                                  # rows 511 and 512 are both heads
    assert any(head[j] and j % c["chunk"] == 0 for j in range(len(keys))) and head[len(keys) - 70] and not head[-1]
    f, mod = MergedFleet(sim, n_streams, "All Messages", "None", slots=16384), Models()
    feed(f, mod, pairs, rng)
    got_keys = np.zeros(len(keys) + 8, np.uint64)
    for grid in (1, 5):
        rc, r, info, n, nk = f.merged_rc(grid=grid, keys=got_keys)
        assert rc == 0 and nk == len(keys) and np.array_equal(got_keys[:nk], keys) and n == 82
        same((r[:n], info[:n]), fold(mod, range(n_streams)), grid)
    cut = 5003
    exp = fold(mod, range(n_streams), cut)
    assert 60 < len(exp[0]) <= 82 and (exp[1]["n_streams"] < 70).any()
    same(f.merged(cutoff=cut), exp)
    sel = list(range(3, 70, 2))
    same(f.merged(sel, cut, grid=2), fold(mod, sel, cut))
    f.close()


def test_stream_bits_above_the_low_nibbles(sim):
    """5000 open streams, three in use: 0, 4097 (bit 12) and 4999, selected as a list and by NULL."""
    rng = np.random.default_rng(82)
    f, mod = MergedFleet(sim, 5000, "All Messages", "None"), Models()
    addr = [0, 0xFFFFFF] + [0x200000 + 4099 * k for k in range(30)]
    use = [0, 4097, 4999]
    feed(f, mod, [(s, a) for s in use for a in addr if (a + s) % 5], rng)
    exp = fold(mod, use)
    assert len(exp[0]) == len(addr) and set(np.unique(exp[1]["src_callsign"])) >= {0, 4097, 4999}
    same(f.merged(use), exp)
    same(f.merged(None), exp)
    same(f.merged([4097, 4999]), fold(mod, [4097, 4999]))
    same(f.merged([1, 2, 4096, 4098]), fold(mod, []))
    f.close()


def test_what_does_not_contribute(sim):
    """A reset stream (before and after the next rehash), expired planes, an announced address without a plane, an unselected
    stream, an empty selection and an empty fleet."""
    rng = np.random.default_rng(83)
    f, mod = MergedFleet(sim, 4, "Extended Squitter Only", "None"), Models("Extended Squitter Only", "None")
    assert f.merged()[0].size == 0 and f.merged([])[0].size == 0 and f.merged([2], 17)[1].size == 0       # an empty fleet
    addr = [0x300000 + 3 * k for k in range(20)]
    feed(f, mod, [(s, a) for s in range(4) for a in addr[s:]], rng)
    ghost = 0x3FFFF0                        # "Extended Squitter Only": a DF 11 reply announces its address and makes no plane
    b, t, s = np.array([TE.df11(ghost)] * 2), np.array([5010.5, 5011.5]), np.array([0, 2], np.int32)
    f.call(b, t, s)
    mod.call(b, t, s)
    assert f.slot_of(0, ghost) >= 0 and ghost not in f.merged()[0]["icao"]
    same(f.merged(), fold(mod, range(4)))
    same(f.merged([0, 1, 3]), fold(mod, [0, 1, 3]))                                          # stream 2 is not selected
    assert f.merged([])[0].size == 0 and f.merged([], 0)[1].size == 0
    f.reset(1)
    mod[1] = TE.Model(*mod.cfg)
    taken = f.taken()
    exp = fold(mod, range(4))
    assert (exp[1]["n_streams"] <= 3).all()
    same(f.merged(), exp, "reset")
    assert f.taken() == taken > f.stats()["planes"]                                          # the stale slots are still there
    assert f.expire([INT64_MIN] * 4) == 0 and f.taken() < taken                              # ... and gone after a rehash
    same(f.merged(), exp, "reset, rehashed")
    n = mod[0].sweep(5003) + mod[3].sweep(5002)
    assert n > 5 and f.expire([5003, 5002], [0, 3]) == n
    same(f.merged(), fold(mod, range(4)), "expired")
    same(f.merged(cutoff=5004), fold(mod, range(4), 5004))
    feed(f, mod, [(1, a) for a in addr[:7]], rng, t0=6000.5)                                 # the reset stream hears again
    same(f.merged(), fold(mod, range(4)), "heard again")
    f.close()


def test_growth_and_same_size_rehash_change_nothing(sim):
    rng = np.random.default_rng(84)
    f, mod = MergedFleet(sim, 3, "All Messages", "Conservative"), Models("All Messages", "Conservative")
    addr = [0x500000 + 17 * k for k in range(40)]
    feed(f, mod, [(s, a) for s in (0, 1) for a in addr], rng)
    before = f.merged([0, 1], 5002)
    same(before, fold(mod, [0, 1], 5002))
    cap = f.stats()["capacity"]
    feed(f, mod, [(2, 0x900000 + k) for k in range(cap // 2)], rng, t0=7000.5)               # the store grows
    assert f.stats()["capacity"] > cap and f.stats()["grows"] >= 1
    same(f.merged([0, 1], 5002), before, "growth")
    assert f.expire([INT64_MIN] * 3) == 0                                                    # a rehash into the same size
    same(f.merged([0, 1], 5002), before, "rehash")
    same(f.merged(), fold(mod, range(3)))
    f.close()


def test_store_at_its_fill_limit(sim):
    """256 slots, 95 planes, a probe cluster that wraps from slot 255 to slot 0 (test_expire.test_fleet_store_at_its_minimum's)."""
    rng = np.random.default_rng(85)
    f, mod = MergedFleet(sim, 3, "All Messages", "None"), Models()
    clus = TE.cluster_addresses(f, 30)
    shared = [0x700000 + 11 * k for k in range(25)]
    pairs = [(0, a) for a in clus] + [(0, a) for a in shared] + [(1, a) for a in shared] + [(2, a) for a in shared[:15]]
    b, t, s = [TE.ident(a, rng) for _, a in pairs], [5000.5 + k % 7 for k in range(len(pairs))], [s for s, _ in pairs]
    f.call(b, t, s)
    mod.call(b, t, s)
    for lo in range(0, len(pairs), 16):                     # more fields for the same planes, 32 records a call at the most:
        feed(f, mod, pairs[lo:lo + 16], rng)                # (slots taken + records) * 2 stays within the 256 slots
    assert f.stats() == dict(planes=95, capacity=256, grows=0, used=95)
    slots = [f.slot_of(0, a) for a in clus]
    assert max(slots) == 255 and min(slots) == 0
    for sel, cut in ((None, INT64_MIN), (None, 5003), ([0, 2], 5002), ([1], INT64_MIN)):
        same(f.merged(sel, cut), fold(mod, range(3) if sel is None else sel, cut), (sel, cut))
    f.close()


def test_one_stream_is_its_own_snapshot_and_nothing_changes(sim):
    """Every stream of a small fleet selected alone: the rows are adsb_stream_planes_seen's, info.last_seen its last_seen,
    n_streams 1, every src_* that stream or -1.  Two merged calls are byte-identical, the snapshot around them is, the store and
    the clocks are, and rows decoded afterwards are those of a fleet that never merged."""
    rng = np.random.default_rng(86)
    f, g_ = MergedFleet(sim, 4, "All Messages", "Conservative"), MergedFleet(sim, 4, "All Messages", "Conservative")
    addr = [0x440000 + 5 * k for k in range(30)]
    b, t = S.mixed(rng, n=500, addresses=addr, t0=7000.5)
    ss = rng.integers(0, 4, len(b)).astype(np.int32)
    S.assert_rows_equal(f.call(b[:300], t[:300], ss[:300]), g_.call(b[:300], t[:300], ss[:300]))
    before = f.snapshot()
    for s in range(4):
        rows, info = f.merged([s])
        srows, sseen, _ = f.snapshot([s])
        TP.rows_equal(rows, srows)
        assert np.array_equal(info["last_seen"], sseen) and (info["n_streams"] == 1).all() and not info["pad"].any()
        for name, flag in zip(SRC[:3], (N.DEC_HAS_CALLSIGN, N.DEC_HAS_ALTITUDE, N.DEC_HAS_VELOCITY)):
            assert np.array_equal(info[name], np.where(rows["present"] & flag, s, -1)), (s, name)
        assert np.array_equal(info["src_position"], np.where(np.isnan(rows["latitude"]), -1, s))
    a, c = f.merged(cutoff=7010), f.merged(cutoff=7010)
    same(a, c)
    assert len(a[0]) and (a[1]["n_streams"] > 1).any()
    after = f.snapshot()
    TP.rows_equal(before[0], after[0])
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert f.stats() == g_.stats() and f.taken() == g_.taken()
    S.assert_rows_equal(f.call(b[300:], t[300:], ss[300:]), g_.call(b[300:], t[300:], ss[300:]))
    x, y = f.snapshot(), g_.snapshot()
    TP.rows_equal(x[0], y[0])
    assert np.array_equal(x[1], y[1])
    same(f.merged(), g_.merged())
    f.close(); g_.close()


def test_cap_rules_and_selections(sim):
    rng = np.random.default_rng(87)
    f, mod = MergedFleet(sim, 3, "All Messages", "None"), Models()
    feed(f, mod, [(s, 0x600000 + a) for s in range(3) for a in range(9 + s)], rng)
    exp = fold(mod, range(3))
    n = len(exp[0])
    assert n == 11
    rc, r, info, got, _ = f.merged_rc(cap=0)                                                 # the count query
    assert (rc, got) == (-28, n)
    rc, r, info, got, _ = f.merged_rc(cap=n - 1)                                             # too small: the count, nothing written
    assert (rc, got) == (-28, n) and (r.view(np.uint8) == 0x77).all() and (info.view(np.uint8) == 0x77).all()
    rc, r, info, got, _ = f.merged_rc(cap=n + 3)
    assert (rc, got) == (0, n) and (r[n:].view(np.uint8) == 0x77).all() and (info[n:].view(np.uint8) == 0x77).all()
    same((r[:n], info[:n]), exp)
    rc, r, info, got, _ = f.merged_rc(cap=n, info=False)                                     # rows alone
    assert rc == 0 and (info.view(np.uint8) == 0x77).all()
    TP.rows_equal(r[:n], exp[0])
    rc, r, info, got, _ = f.merged_rc(cap=n, rows=False)                                     # info alone
    assert rc == 0 and (r.view(np.uint8) == 0x77).all() and info[:n].tobytes() == exp[1].tobytes()
    assert f.merged_rc(cap=n, rows=False, info=False)[0] == -22
    for bad in ([2, 1], [0, 0], [3], [-1]):
        assert f.merged_rc(bad)[0] == -22, bad
    f.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
class EmulatedLib:
    """libadsb_hip.so's adsb_stream_planes_merged, answered by the emulated kernels; calls: (cap, rc) of every call"""

    def __init__(self, fleet):
        self.fleet, self.calls = fleet, []

    def adsb_stream_planes_merged(self, h, streams, n_sel, cutoff, rows, info, cap, n_out):
        n = ctypes.c_int(-1)
        rc = self.fleet.lib.sim_merge_fleet(self.fleet.h, streams, ctypes.c_int(n_sel), ctypes.c_longlong(cutoff), ctypes.c_int(3),
                                            ctypes.c_int(cap), rows, info, ctypes.byref(n), None, None)
        ctypes.cast(n_out, ctypes.POINTER(ctypes.c_int32))[0] = n.value
        self.calls.append((cap, rc))
        return rc

    def adsb_last_error(self, h):
        return b"emulated"


class EmulatedContext(N.Context):
    """_native.Context's own merged_planes over EmulatedLib; what frontend.Receivers asks beside it"""

    def __init__(self, fleet, flags):
        self.lib, self._h, self.flags = EmulatedLib(fleet), fleet.h, flags

    def open_streams(self, n):
        assert n == self.fleet_n
        self._streams_open = n

    def close(self):
        pass


def test_python_layer(sim):
    from gr_adsb_amd import frontend
    rng = np.random.default_rng(88)
    f, mod = MergedFleet(sim, 4, "All Messages", "None"), Models()
    feed(f, mod, [(s, 0x0A0000 + 3 * a) for s in range(4) for a in range(6 + s)], rng, t0=1760000000.5)
    ctx = EmulatedContext(f, N.FLAG_STREAM_DECODE | N.FLAG_PLANE_AGES)
    ctx.fleet_n = 4
    rx = frontend.Receivers(ctx, 4, ages=True)
    same(ctx.merged_planes(), fold(mod, range(4)))
    assert ctx.lib.calls == [(0, -28), (9, 0)]                                               # a count query first
    same(ctx.merged_planes(cap=64), fold(mod, range(4)))
    assert ctx.lib.calls[2:] == [(64, 0)]
    same(ctx.merged_planes([1, 3], 1760000003), fold(mod, [1, 3], 1760000003))
    same(ctx.merged_planes([], None), fold(mod, []))
    with pytest.raises(ValueError):
        ctx.merged_planes([3, 1])
    with pytest.raises(ValueError):
        ctx.merged_planes([4])
    rows, info = rx.merged()
    same((rows, info), fold(mod, range(4)))
    same(rx.merged([0, 2], cutoff=1760000002), fold(mod, [0, 2], 1760000002))
    assert rx.table(1760000100.0) == N.plane_table(rows, 1760000100.0) and len(rx.table(1760000100.0)) == 9
    assert rx.table(1760000100.0, ids=[3], cutoff=1760000001) == N.plane_table(fold(mod, [3], 1760000001)[0], 1760000100.0)
    d = N.plane_entry(rows[0], info["last_seen"][0])
    assert d["last_seen"] == int(info["last_seen"][0]) and d["num_msgs"] == int(rows["num_msgs"][0])
    # refusals: no ages, no decoders
    plain = EmulatedContext(f, N.FLAG_STREAM_DECODE)
    plain.fleet_n = 4
    with pytest.raises(ValueError):
        frontend.Receivers(plain, 4).merged()
    with pytest.raises(ValueError):
        frontend.Receivers(plain, 4).table(0.0)
    none = EmulatedContext(f, 0)
    none.fleet_n = 4
    with pytest.raises(ValueError):
        frontend.Receivers(none, 4).merged()
    f.close()


def test_symbol_dtype_and_abi():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert N.MERGED_DTYPE.itemsize == 32 and N.MERGED_DTYPE.names == ("last_seen", "n_streams") + SRC + ("pad",)
    assert [N.MERGED_DTYPE.fields[k][1] for k in N.MERGED_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]
    assert N.INT64_MIN == INT64_MIN
    assert "adsb_stream_planes_merged" in N.EXPORTS and re.search(r"^int adsb_stream_planes_merged\(adsb_ctx\* ctx", src, re.M)
    assert re.search(r"typedef struct adsb_merged \{", src) and re.search(r"#define ADSB_ABI_VERSION 5\b", src) and N.ABI_VERSION == 5
    dev = open(os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")).read()
    host = open(os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_hip.hip")).read()
    assert "static_assert(sizeof(MergedInfo) == 32" in dev and "static_assert(sizeof(adsb_merged) == 32" in host
    from gr_adsb_amd import frontend
    assert callable(N.Context.merged_planes) and callable(frontend.Receivers.merged) and callable(frontend.Receivers.table)


def test_library_exports_the_symbol():
    lib = N.load()
    assert lib.adsb_stream_planes_merged is not None and lib.adsb_abi_version() == 5


RECORD = ("agprs", "lds_bytes_per_block", "occupancy_waves_per_simd", "scratch_bytes_per_lane", "sgpr_spills", "sgprs", "vgpr_spills",
          "vgprs")


def test_kernel_resources():
    """The new kernels exist and have no LDS, no scratch and no spills; every kernel the parent had has the parent's record
    (tests/golden/merge_parent_kernels.json: the parent's kernel_resources.json, RECORD's fields in that order)."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    new = {k: v for k, v in res.items() if "k_merge_" in k}
    names = sorted(re.search(r"k_merge_[a-z_]+?(?=E)", k).group(0) for k in new)
    assert names == ["k_merge_emit", "k_merge_heads", "k_merge_keys"], sorted(new)
    for k, v in new.items():
        assert v["lds_bytes_per_block"] == 0 and v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    parent = json.load(open(PARENT_KERNELS))
    assert len(parent) == 98 and sorted(parent) == sorted(k for k in res if k not in new)
    for k, rec in parent.items():
        assert [res[k][f] for f in RECORD] == rec, (k, res[k], rec)
