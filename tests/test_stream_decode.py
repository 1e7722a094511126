"""ADSB_FLAG_STREAM_DECODE on the CPU: one decoder behind every receiver stream, one sparse store for all of them.  The
emulated kernels (tests/sim/fleet_driver.cpp: k_fleet_*, the library's own sort, the host's growth rule) against one
plain-Python replay PER STREAM (tests/decode_replay.py, pinned to the reference by tests/golden/g_decode.npz in
tests/test_decode.py), the kernels' resources and the constants of the interface.

What a green run here does NOT cover: the driver restates the host's growth, reset and bookkeeping rules (adsb_hip.hip
fleet_step / fleet_rehash / fleet_reset_stream) instead of running them, and its clock is whole seconds at fs = 1.  The host
code itself, and start + (double)offset / fs with fractional starts, are covered by tests/test_gpu_stream_decode.py only."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
FLEET_SO = os.path.join(SIM_DIR, "libadsb_fleet_sim.so")
GOLD = os.path.join(HERE, "golden", "g_decode.npz")
CONFIGS = (("All Messages", "None"), ("All Messages", "Conservative"), ("Extended Squitter Only", "None"))
SORT_TILE = 4096
MIN_CAP = 256


def fleet_lib():
    srcs = [os.path.join(SIM_DIR, "fleet_driver.cpp"), os.path.join(SIM_DIR, "sim_support.h"), os.path.join(SIM_DIR, "hipsim.h"),
            os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not (os.path.exists(FLEET_SO) and all(os.path.getmtime(FLEET_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", FLEET_SO])
    lib = ctypes.CDLL(FLEET_SO)
    lib.sim_fleet_open.restype = ctypes.c_void_p
    lib.sim_fleet_taken.restype = ctypes.c_longlong
    lib.sim_fleet_gen_max.restype = ctypes.c_uint
    lib.sim_fleet_get_call.restype = ctypes.c_ulonglong
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = fleet_lib()
    assert lib.sim_fleet_row_bytes() == N.DECODED_DTYPE.itemsize
    assert lib.sim_fleet_slot_bytes() == 104 and lib.sim_fleet_sort_tile() == SORT_TILE
    return lib


class SimFleet:
    """The decoders of n streams on the emulated kernels: the store and the host's bookkeeping live in the driver."""

    def __init__(self, lib, n_streams, filt, corr, slots=1 << 16, starts=None):
        self.lib = lib
        self.h = ctypes.c_void_p(lib.sim_fleet_open(ctypes.c_int(n_streams), ctypes.c_longlong(slots),
                                                    ctypes.c_int(corr == "Conservative"), ctypes.c_int(filt == "All Messages")))
        for s, t in enumerate(starts if starts is not None else []):
            lib.sim_fleet_set_start(self.h, ctypes.c_int(s), ctypes.c_double(t))

    def close(self):
        self.lib.sim_fleet_close(self.h)

    def call(self, bits14, ts, stream, grid=3):
        b = np.ascontiguousarray(bits14, dtype=np.uint8)
        t = np.ascontiguousarray(ts, dtype=np.float64)
        s = np.ascontiguousarray(stream, dtype=np.int32)
        rows = np.zeros(len(b), dtype=N.DECODED_DTYPE)
        vp = ctypes.c_void_p
        rc = self.lib.sim_fleet_call(self.h, b.ctypes.data_as(vp), t.ctypes.data_as(vp), s.ctypes.data_as(vp), ctypes.c_int(len(b)),
                                     ctypes.c_int(grid), rows.ctypes.data_as(vp))
        assert rc == 0, "guard word overwritten (-1), sorted key names nothing (-2), error word / claims miscounted (-3): %d" % rc
        return rows

    def reset(self, stream):
        assert self.lib.sim_fleet_reset(self.h, ctypes.c_int(stream)) == 0

    def set_gen(self, stream, gen):
        self.lib.sim_fleet_set_gen(self.h, ctypes.c_int(stream), ctypes.c_uint(gen))

    def stats(self):
        v = [ctypes.c_longlong() for _ in range(4)]
        self.lib.sim_fleet_stats(self.h, *[ctypes.byref(x) for x in v])
        return dict(planes=v[0].value, capacity=v[1].value, grows=v[2].value, used=v[3].value)

    def taken(self):
        return int(self.lib.sim_fleet_taken(self.h))


class Replays:
    """One decode_replay.Decoder per stream: the expectation, call by call."""

    def __init__(self, n_streams, filt, corr):
        self.cfg = (filt, corr)
        self.dec = [D.Decoder(filt, corr) for _ in range(n_streams)]

    def call(self, bits14, ts, stream):
        return S.to_rows([self.dec[int(s)].row(b, t) for b, t, s in zip(bits14, ts, stream)])

    def reset(self, stream):
        self.dec[stream] = D.Decoder(*self.cfg)

    def planes(self):
        return sum(len(d.planes) for d in self.dec)


def interleave(streams):
    """[(bits14, ts)] per stream -> (bits14, ts, stream index) in timestamp order (stable: a stream's PDUs keep their order)."""
    b = np.concatenate([x[0] for x in streams])
    t = np.concatenate([x[1] for x in streams])
    s = np.concatenate([np.full(len(x[1]), k, np.int32) for k, x in enumerate(streams)])
    order = np.argsort(t, kind="stable")
    return b[order], t[order], s[order]


def cuts(rng, n, lo, hi):
    out, i = [], 0
    while i < n:
        k = min(int(rng.integers(lo, hi + 1)), n - i)
        out.append((i, i + k))
        i += k
    return out


# ---- isolation traffic -------------------------------------------------------------------------------------------------------
ISO_ADDR = [0, 0xFFFFFF] + [0x400000 + 17 * k for k in range(38)]
_iso = {}


def iso_traffic():
    if "t" not in _iso:
        _iso["t"] = interleave([S.mixed(np.random.default_rng(100 + s), n=1200, addresses=ISO_ADDR, t0=1760000000.5 + 0.37 * s,
                                        dt=(0.002, 0.05)) for s in range(3)])
    return _iso["t"]


def iso_expected(filt, corr):
    """Per-stream replay rows of the isolation traffic, with the two facts that keep the test from going blind."""
    if (filt, corr) not in _iso:
        b, t, s = iso_traffic()
        rep = Replays(3, filt, corr)
        exp = rep.call(b, t, s)
        for k in range(3):
            assert (exp["port"][s == k] == D.DECODED).sum() >= 600 and len(rep.dec[k].planes) == 40
        shared = S.to_rows(D.Decoder(filt, corr).rows(b, t))
        differ = np.any(shared.view(np.uint8).reshape(len(b), -1) != exp.view(np.uint8).reshape(len(b), -1), axis=1).sum()
        assert differ >= 1000, differ
        _iso[(filt, corr)] = exp, rep.planes()
    return _iso[(filt, corr)]


@pytest.mark.parametrize("filt,corr", CONFIGS)
def test_streams_that_share_addresses_decode_alone(sim, filt, corr):
    """Three streams of the same 40 aircraft, interleaved by timestamp into calls of 1-400 PDUs: every stream's rows are those of
    a decoder of its own, which one decoder for all three would not give."""
    b, t, s = iso_traffic()
    exp, planes = iso_expected(filt, corr)
    f = SimFleet(sim, 3, filt, corr, starts=[1760000000.5 + 0.37 * k for k in range(3)])
    rng = np.random.default_rng(7)
    got = np.concatenate([f.call(b[lo:hi], t[lo:hi], s[lo:hi], grid=int(rng.integers(1, 4))) for lo, hi in cuts(rng, len(b), 1, 400)])
    S.assert_rows_equal(got, exp)
    st = f.stats()
    assert st["planes"] == planes == 120 and st["grows"] == 0
    f.close()


# ---- growth and probing ------------------------------------------------------------------------------------------------------
def test_store_grows_from_its_minimum_without_changing_a_row(sim):
    """About 1500 (stream, address) pairs over several calls into a store reserved at its minimum: several growths, the plane
    count that of the replays after every call, rows unchanged.  Stream 0 and the last stream, addresses 0 and 0xFFFFFF."""
    n_streams = 8
    addr = [0, 0xFFFFFF] + [0x500000 + 4099 * k for k in range(188)]
    b, t, s = interleave([S.mixed(np.random.default_rng(200 + k), n=700, addresses=addr, t0=1760000100.25 + 0.11 * k, dt=(0.002, 0.05))
                          for k in range(n_streams)])
    for filt, corr in CONFIGS[:2]:
        rep = Replays(n_streams, filt, corr)
        f = SimFleet(sim, n_streams, filt, corr, slots=0, starts=[1760000100.25 + 0.11 * k for k in range(n_streams)])
        assert f.stats()["capacity"] == MIN_CAP
        rng = np.random.default_rng(8)
        caps = [MIN_CAP]
        for lo, hi in cuts(rng, len(b), 150, 450):
            got = f.call(b[lo:hi], t[lo:hi], s[lo:hi])
            S.assert_rows_equal(got, rep.call(b[lo:hi], t[lo:hi], s[lo:hi]))
            st = f.stats()
            assert st["planes"] == rep.planes()
            assert 2 * st["used"] <= st["capacity"] and f.taken() == st["used"]
            caps.append(st["capacity"])
        assert 1400 <= rep.planes() <= n_streams * len(addr) == 1520
        assert st["grows"] >= 3 and st["grows"] == len(set(caps)) - 1 and all(c & (c - 1) == 0 for c in caps)
        assert {0, n_streams - 1} <= set(s.tolist())
        f.close()


def test_noise_takes_no_slots(sim):
    """3000 random 112-bit rows behind five aircraft: address/parity replies with unheard addresses by the thousand, and not
    one slot more than the replay has planes."""
    rng = np.random.default_rng(9)
    b0, t0 = S.mixed(np.random.default_rng(10), n=120, addresses=[0x111111, 0x222222, 0x333333, 0x444444, 0x555555])
    noise = rng.integers(0, 256, (3000, 14)).astype(np.uint8)
    tn = float(t0[-1]) + np.cumsum(rng.uniform(0.001, 0.01, 3000))
    ap = np.isin(noise[:, 0] >> 3, (0, 4, 5, 16, 20, 21, 24)).sum()
    assert ap > 500
    for filt, corr in CONFIGS[:2]:
        rep = Replays(2, filt, corr)
        f = SimFleet(sim, 2, filt, corr, slots=0)
        z0, zn = np.zeros(len(b0), np.int32), np.zeros(3000, np.int32)
        S.assert_rows_equal(f.call(b0, t0, z0), rep.call(b0, t0, z0))
        before = f.taken()
        S.assert_rows_equal(f.call(noise, tn, zn), rep.call(noise, tn, zn))
        st = f.stats()
        assert st["planes"] == rep.planes() and f.taken() == rep.planes()      # "All Messages": every slot holds a plane
        assert f.taken() - before <= 2
        f.close()


# ---- more than one sort tile -------------------------------------------------------------------------------------------------
BUSY = 0x5A5A5A
_large = {}


def large_call():
    """About 9000 PDUs of two streams in timestamp order: 5000 of one aircraft of stream 0 among 2000 of 1000 others, and 2000
    of stream 1, which hears the busy aircraft's address too."""
    if "c" not in _large:
        others = [0, 0xFFFFFF] + [0x300000 + 4099 * k for k in range(998)]
        a = S.mixed(np.random.default_rng(31), n=5000, addresses=[BUSY], dt=(0.002, 0.2))
        o = S.mixed(np.random.default_rng(32), n=2000, addresses=others, dt=(0.005, 0.5))
        order = np.argsort(np.concatenate([a[1], o[1]]), kind="stable")
        s0 = np.concatenate([a[0], o[0]])[order], np.concatenate([a[1], o[1]])[order]
        s1 = S.mixed(np.random.default_rng(33), n=2000, addresses=[BUSY] + others[:300], dt=(0.005, 0.5))
        _large["c"] = interleave([s0, s1])
    return _large["c"]


@pytest.mark.parametrize("filt,corr", CONFIGS[:2])
def test_one_call_over_several_sort_tiles(sim, filt, corr):
    """More than two tiles of keys in one call; the busy aircraft's slot segment alone is longer than a tile."""
    b, t, s = large_call()
    exp = Replays(2, filt, corr).call(b, t, s)
    assert len(b) >= 9000 and exp["num_msgs"][(exp["icao"] == BUSY) & (s == 0)].max() > SORT_TILE + 200
    assert exp["num_msgs"][(exp["icao"] == BUSY) & (s == 1)].max() < 100
    f = SimFleet(sim, 2, filt, corr)
    S.assert_rows_equal(f.call(b, t, s, grid=4), exp)
    f.close()


# ---- reset -------------------------------------------------------------------------------------------------------------------
def test_reset_of_one_stream_leaves_the_others(sim):
    """adsb_stream_reset between calls: that stream's rows restart, the others go on; its planes leave the count at once and its
    slots leave the store with the next growth.  The same when the stream's generations are used up (a rehash at the reset)."""
    filt, corr = CONFIGS[0]
    addr = [0xA00000 + k for k in range(60)]
    b, t, s = interleave([S.mixed(np.random.default_rng(300 + k), n=500, addresses=addr, t0=1760000200.5 + k, dt=(0.002, 0.05))
                          for k in range(3)])
    third = len(b) // 3
    rep = Replays(3, filt, corr)
    f = SimFleet(sim, 3, filt, corr, slots=0)
    f.set_gen(2, sim.sim_fleet_gen_max())
    sl = slice(0, third)
    S.assert_rows_equal(f.call(b[sl], t[sl], s[sl]), rep.call(b[sl], t[sl], s[sl]))
    all3 = rep.planes()
    of1, of2 = len(rep.dec[1].planes), len(rep.dec[2].planes)
    assert f.stats()["planes"] == all3 == f.taken() and min(of1, of2) >= 40        # "All Messages": every slot holds a plane
    f.reset(1)
    rep.reset(1)
    assert f.stats()["planes"] == rep.planes() == all3 - of1 and f.taken() == all3       # stale slots stay until a rehash
    sl = slice(third, 2 * third)
    got, exp = f.call(b[sl], t[sl], s[sl]), rep.call(b[sl], t[sl], s[sl])
    S.assert_rows_equal(got, exp)
    first = np.flatnonzero((s[sl] == 1) & (got["present"] != 0))[0]
    kinds = N.DEC_HAS_CALLSIGN | N.DEC_HAS_ALTITUDE | N.DEC_HAS_VELOCITY
    assert got["num_msgs"][first] == 1 and bin(int(got["present"][first]) & kinds).count("1") <= 1      # one message's worth
    assert got["num_msgs"][np.flatnonzero((s[sl] == 0) & (got["present"] != 0))[0]] > 1                 # the others went on
    # more addresses on stream 0: the store grows and drops what the reset left behind
    b2, t2 = S.mixed(np.random.default_rng(310), n=1600, addresses=[0xB00000 + k for k in range(900)], t0=float(t[2 * third]))
    z = np.zeros(len(b2), np.int32)
    g0 = f.stats()["grows"]
    S.assert_rows_equal(f.call(b2, t2, z), rep.call(b2, t2, z))
    st = f.stats()
    assert st["grows"] > g0 and st["planes"] == rep.planes() == f.taken() > all3
    # stream 2 has used up its generations: its reset rehashes the store at once
    before, of2 = rep.planes(), len(rep.dec[2].planes)
    f.reset(2)
    rep.reset(2)
    assert f.stats()["planes"] == rep.planes() == f.taken() == before - of2
    sl = slice(2 * third, len(b))
    S.assert_rows_equal(f.call(b[sl], t[sl], s[sl]), rep.call(b[sl], t[sl], s[sl]))
    assert f.stats()["planes"] == rep.planes() == f.taken()
    f.close()


def test_periodic_resets_do_not_grow_the_store(sim):
    """The same 100 aircraft on one stream, reset after every round: the slots the resets leave behind are dropped by a rehash
    at the SAME capacity, which is no growth -- the capacity follows the live slots, not the slots ever claimed."""
    filt, corr = CONFIGS[0]
    b, t = S.mixed(np.random.default_rng(400), n=300, addresses=[0xC00000 + k for k in range(100)])
    z = np.zeros(len(b), np.int32)
    f = SimFleet(sim, 2, filt, corr, slots=0)
    exp = Replays(1, filt, corr).call(b, t, z)
    seen = []
    for _ in range(8):
        S.assert_rows_equal(f.call(b, t, z), exp)
        st = f.stats()
        seen.append((st["capacity"], st["grows"], f.taken()))
        f.reset(0)
    assert (exp["present"] != 0).sum() > 200
    # round 0 grows to hold 300 records' worth; 8 rounds claim about 800 slots, far more than half of that store
    assert len({c for c, _, _ in seen}) == 1 and len({g for _, g, _ in seen}) == 1 and seen[0][0] <= 1024
    assert max(k for _, _, k in seen) * 2 <= seen[0][0] and sum(k for _, _, k in seen[:1]) * 8 > seen[0][0] // 2
    f.close()


def test_call_numbers_start_over_before_they_run_out(sim):
    """The ordering keys hold the call's number in 32 bits.  Just before it runs out a rehash gives every announcement made so
    far key 0 and the numbering starts at 1: address/parity replies of aircraft heard before are still known afterwards."""
    for filt, corr in CONFIGS[:2]:
        b, t = S.mixed(np.random.default_rng(410), n=600, addresses=[0xD00000 + k for k in range(30)])
        s = (np.arange(len(b)) % 2).astype(np.int32)
        rep = Replays(2, filt, corr)
        f = SimFleet(sim, 2, filt, corr)
        sim.sim_fleet_set_call(f.h, ctypes.c_ulonglong(0xFFFFFFFC))
        got, nums = [], []
        for lo in range(0, len(b), 100):
            got.append(f.call(b[lo:lo + 100], t[lo:lo + 100], s[lo:lo + 100]))
            nums.append(int(sim.sim_fleet_get_call(f.h)))
        exp = rep.call(b, t, s)
        S.assert_rows_equal(np.concatenate(got), exp)
        assert nums == [0xFFFFFFFD, 0xFFFFFFFE, 2, 3, 4, 5] and f.stats()["grows"] == 0
        late = np.arange(len(b)) >= 200
        ap_rows = late & np.isin(exp["df"], (0, 4, 5, 16, 20, 21)) & (exp["present"] != 0)
        assert ap_rows.sum() > 30                       # accepted because their AA was announced before the renumbering
        f.close()


# ---- CPR and the decoder's clock ---------------------------------------------------------------------------------------------
def seq_slices(seq):
    cut = np.flatnonzero(np.diff(seq)) + 1
    b = np.concatenate([[0], cut, [len(seq)]])
    return [slice(int(b[i]), int(b[i + 1])) for i in range(len(b) - 1)]


def position(aa, lat, lon, odd):
    la, lo = S.cpr_encode(lat, lon, odd)
    body = np.zeros(51, np.uint8)
    body[3:15], body[16], body[17:34], body[34:51] = S.ib(0xC38, 12), odd, S.ib(la, 17), S.ib(lo, 17)
    return np.packbits(S.es(aa, 11, body))


def test_cpr_pairs_across_calls_and_the_30_s_limit(sim):
    """The golden's long sequences, one per stream with its own start, in calls of 1-40 PDUs: even and odd frames of a pair lie in
    different calls.  And a hand-made aircraft per stream: an even frame, an odd one 10 s later (a fix), an even one 45 s after
    that (no fix: the odd frame is too old by the PDU timestamps), each in a call of its own."""
    g = np.load(GOLD)
    sls = [sl for sl in seq_slices(g["seq"]) if sl.stop - sl.start >= 60]
    assert len(sls) >= 4
    streams = [(g["bits"][sl], g["ts"][sl] + 1000.25 * k) for k, sl in enumerate(sls)]
    b, t, s = interleave(streams)
    for filt, corr in (CONFIGS[0], CONFIGS[1]):
        rep = Replays(len(sls) + 1, filt, corr)
        f = SimFleet(sim, len(sls) + 1, filt, corr, starts=[float(x[1][0]) - 0.75 for x in streams] + [0.0])
        rng = np.random.default_rng(12)
        got = np.concatenate([f.call(b[lo:hi], t[lo:hi], s[lo:hi]) for lo, hi in cuts(rng, len(b), 1, 40)])
        exp = rep.call(b, t, s)
        S.assert_rows_equal(got, exp)
        fix = ~np.isnan(exp["latitude"])
        assert fix.sum() > 100 and len(set(s[fix].tolist())) >= 2
        k = len(sls)
        for base in (1760000000.9, 1760000000.1):
            frames = [(position(0xC0FFEE, 48.1, 11.5, 0), base), (position(0xC0FFEE, 48.1, 11.5, 1), base + 10.0),
                      (position(0xC0FFEE, 48.1, 11.5, 0), base + 55.0), (position(0xC0FFEE, 48.1, 11.5, 1), base + 84.2)]
            rows = []
            for fb, ft in frames:
                one = f.call(fb[None, :], [ft], [k])
                S.assert_rows_equal(one, rep.call(fb[None, :], [ft], [k]))
                rows.append(one[0])
            # alone: no fix; 10 s apart: the first fix (not published: nothing to compare it with); 45 s after the odd frame: no
            # fix; then 29.2 s after the even one, which is 30 whole seconds of the decoder's clock from x.9 and 29 from x.1
            assert [int(r["port"]) for r in rows] == [D.NONE, D.NONE, D.NONE, D.NONE if base % 1 > 0.5 else D.DECODED]
            assert np.isnan(rows[0]["latitude"])
            assert not np.isnan(rows[1]["latitude"])
            f.reset(k)
            rep.reset(k)
        f.close()


# ---- resources ---------------------------------------------------------------------------------------------------------------
def test_kernel_resources_fit_beside_every_k_detect():
    """Every kernel of the per-stream decoders: no scratch, no spills, and room for a workgroup beside every k_detect instance
    (the arithmetic of tests/test_decode.py)."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    LDS_CU, VGPR_SIMD, SIMDS, GRAN = 160 * 1024, 512, 4, 1280
    alloc = lambda v: -(-v // 8) * 8                                    # noqa: E731
    gran = lambda b: -(-b // GRAN) * GRAN                               # noqa: E731
    fleet = {k: v for k, v in res.items() if "k_fleet" in k}
    names = sorted(re.search(r"k_fleet_[a-z]+", k).group(0) for k in fleet)
    assert names == ["k_fleet_announce", "k_fleet_classify", "k_fleet_cond", "k_fleet_fold", "k_fleet_rehash", "k_fleet_verdict"]
    detect = {k: v for k, v in res.items() if "k_detect" in k}
    assert len(detect) == 35
    for name, d in detect.items():
        mode = int(re.search(r"k_detectILi(\d)E", name).group(1))
        wpb = 1 if mode in (3, 4, 5, 6) else 4
        wg_cu = min(LDS_CU // gran(d["lds_bytes_per_block"]), SIMDS * (VGPR_SIMD // alloc(d["vgprs"])) // wpb, 32)
        free_lds = LDS_CU - wg_cu * gran(d["lds_bytes_per_block"])
        per_simd = [6, 5, 5, 5] if wpb == 1 else [5, 5, 5, 5]
        for fname, f in fleet.items():
            assert f["scratch_bytes_per_lane"] == 0 and f["vgpr_spills"] == 0 and f["sgpr_spills"] == 0, fname
            assert gran(f["lds_bytes_per_block"]) <= free_lds, (fname, name)
            slots = sum((VGPR_SIMD - w * alloc(d["vgprs"])) // alloc(f["vgprs"]) for w in per_simd)
            assert slots >= 4, (fname, f["vgprs"], name, d["vgprs"])


# ---- constants ---------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("adsb_streams_set_decoder", "adsb_stream_set_start", "adsb_stream_last_decoded", "adsb_stream_decoder_reserve",
               "adsb_stream_decoder_stats")


def test_flag_and_abi_constants():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_FLAG_STREAM_DECODE 1024u", src)
    assert N.FLAG_STREAM_DECODE == 1024 and N.ABI_VERSION == 5
    assert re.search(r"#define ADSB_ABI_VERSION 5\b", src)
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS and re.search(r"^int %s\(adsb_ctx\* ctx" % name, src, re.M), name
    for method in ("set_streams_decoder", "set_stream_start", "last_stream_decoded", "stream_decoder_reserve", "stream_decoder_stats"):
        assert callable(getattr(N.Context, method))
