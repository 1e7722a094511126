"""adsb_stream_mlat on the CPU: the emulated kernels of gr_adsb_amd/csrc/adsb_mlat_device.h (tests/sim/mlat_driver.cpp: the
launches in adsb_mlat.hip's order on a carry stated entry by entry, the host's sizing and -ENOSPC rules restated) against the
plain-Python restatement of the header's MULTILATERATION section in tests/mlat_replay.py.  There is no golden from the
reference: it is one receiver and has no counterpart.

Exact: the heads, the member lists, n_rx, n_heard, bits, flags, icao, status, first; iters within 1 (the stopping test sits
on a rounding edge).  Positions: within TOL of the float64 oracle, and -- the arrival times being exact to the double --
within TOL plus the oracle's own distance from the truth of the true position.

TOL.  The float64 oracle against its own np.longdouble run over every case of this file that converges differs by at most
SENS = 5e-7 m (measured: 1.2e-8 m over 97 fixes; test_the_oracles_own_sensitivity prints and bounds it); the device sums the hearings in
another order than the oracle, so 16 x SENS is allowed, and never less than 2e-3 m, twice the stopping threshold:
TOL = max(16 x SENS, 2e-3) = 2e-3 m.

What a green run here does NOT cover: the host's own code (adsb_stream_mlat, adsb_stream_set_ecef and their refusals), the
carry as fleet_step leaves it, and the Python front end -- tests/test_gpu_mlat.py; and everything on the device's side of
these seams: what hipcc makes of __ballot, __shfl, __shfl_up and the LDS staging, the real launchers' grid sizing (the
launches here are the driver's own) and the kernels' second grid-stride round under them, which needs more than 524 288
entries -- tests/test_gpu_mlat_device.py runs this file's cases, unchanged, on the MI355X through
tests/gpu/mlat_device_driver.hip, compares the device's bytes with this emulation's, and adds the large carry."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import mlat_replay as MR
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
MLAT_SO = os.path.join(SIM_DIR, "libadsb_mlat_sim.so")
TILE = 1024                   # entries per LDS tile of k_mlat_heads
SENS = 5e-7                   # m: the bound on the oracle's own float64-vs-longdouble distance over this file's cases
TOL = max(16 * SENS, 2e-3)    # m
T0 = 1000.0                   # s: the ulp of an arrival time is 0.1 ps
WINDOW = 0.002
vp = ctypes.c_void_p
measured = []                 # (case, float64-vs-longdouble distance) of every converged fix compared in this run


def mlat_lib():
    csrc = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, f) for f in ("mlat_driver.cpp", "hipsim.h", "mlat_host_rule.h")] + \
        [os.path.join(csrc, f) for f in ("adsb_mlat_device.h", "adsb_mlat.h", "adsb_dedup_device.h")]
    if not (os.path.exists(MLAT_SO) and all(os.path.getmtime(MLAT_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", MLAT_SO])
    lib = ctypes.CDLL(MLAT_SO)
    lib.sim_mlat_layout_bytes.restype = ctypes.c_ulonglong
    lib.sim_mlat_layout_bytes.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = mlat_lib()
    assert lib.sim_mlat_tile() == TILE and lib.sim_mlat_fix_bytes() == N.MLAT_DTYPE.itemsize == 88
    return lib


# ---- worlds ------------------------------------------------------------------------------------------------------------------
LAT0, LON0 = 52.0, 5.0


def receivers(n, seed=1):
    """n antennas over about 200 km x 200 km of the ellipsoid around (52 N, 5 E), 0 .. 2500 m up -> {stream: ECEF}"""
    rng = np.random.default_rng(seed)
    return {s: tuple(MR.geodetic_to_ecef(LAT0 + rng.uniform(-0.9, 0.9), LON0 + rng.uniform(-1.45, 1.45), rng.uniform(0.0, 2500.0)))
            for s in range(n)}


AIRCRAFT = [MR.geodetic_to_ecef(52.2, 4.7, 9000.0),       # inside the receivers' hull
            MR.geodetic_to_ecef(51.6, 5.9, 1000.0),       # inside, low
            MR.geodetic_to_ecef(53.6, 7.5, 11000.0),      # outside
            MR.geodetic_to_ecef(50.7, 2.9, 12000.0)]      # outside, the other way
# The rule's Gauss-Newton has no damping: with receivers this close to one plane it diverges, or ends on the mirror image below
# them, for about a third of random geometries (measured with the oracle alone).  The cases meant to converge use seeds at
# which the ORACLE converges to the truth -- found on the CPU with tests/mlat_replay.py only, and asserted in check().
RX8 = receivers(8, seed=2)
GOOD_SEED = {4: 73, 5: 18, 8: 3, 63: 3, 64: 3, 65: 3, 130: 3}


def reply(df, seed, long_=None):
    """14 bytes of downlink format df: random but for the format bits"""
    b = np.random.default_rng(1000 * df + seed).integers(0, 256, 14).astype(np.uint8)
    b[0] = (df << 3) | (b[0] & 7)
    return b, (df >= 16) if long_ is None else long_


def arrival(p, rx, s, t_tx):
    return T0 + t_tx + float(np.sqrt(((np.asarray(p) - np.asarray(rx[s])) ** 2).sum())) / MR.C


class Carry:
    """Hearings in any order -> the carry: ascending ts, ties in the order they were added (a stable sort)."""

    def __init__(self):
        self.rows = []

    def add(self, ts, bits, long_, stream, part=True):
        self.rows.append((float(ts), np.asarray(bits, np.uint8), 0 if not part else 2 if long_ else 1, int(stream)))
        return self

    def hear(self, p, rx, streams, t_tx, bits, long_):
        for s in streams:
            self.add(arrival(p, rx, s, t_tx), bits, long_, s)
        return self

    def sorted(self):
        order = sorted(range(len(self.rows)), key=lambda k: self.rows[k][0])
        return [self.rows[k] for k in order]

    def arrays(self):
        r = self.sorted()
        n = len(r)
        return (np.array([x[0] for x in r], np.float64), np.array([x[1] for x in r], np.uint8).reshape(n, 14),
                np.array([x[2] for x in r], np.int32), np.array([x[3] for x in r], np.int32))

    def replay_list(self):
        return [(ts, None if mk == 0 else MR.payload_of(b, mk == 2), s) for ts, b, mk, s in self.sorted()]


def rx_array(rx, n_streams):
    a = np.full((n_streams, 3), np.nan)
    for s, p in rx.items():
        a[s] = p
    return a


def run(sim, carry, rx, **kw):
    """-> (rc, fixes, member_stream, member_ts, heads, n_fixes, n_members)"""
    return run_arrays(sim, *carry.arrays(), rx, **kw)


def run_arrays(sim, ts, bits, mk, stream, rx, n_streams=None, t_lo=-np.inf, t_hi=np.inf, min_rx=4, grid=0, zero_hash=0, cap=None, member_cap=None,
               window=WINDOW):
    """run() over the carry's four arrays, in carry order"""
    nc = len(ts)
    n_streams = n_streams or (max([int(stream.max()) if nc else 0] + list(rx)) + 1)
    rxa = rx_array(rx, n_streams)
    cap = nc // 4 + 1 if cap is None else cap
    member_cap = nc if member_cap is None else member_cap
    fixes = np.zeros(cap, dtype=N.MLAT_DTYPE)
    fixes["first"] = -77                                               # untouched rows stay recognisable
    ms, mt = np.full(member_cap, -77, np.int32), np.full(member_cap, -77.0, np.float64)
    heads = np.zeros(max(nc, 1), np.int32)
    nf, nm, nh = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = sim.sim_mlat(ts.ctypes.data_as(vp), bits.ctypes.data_as(vp), mk.ctypes.data_as(vp), stream.ctypes.data_as(vp), ctypes.c_int(nc),
                      rxa.ctypes.data_as(vp), ctypes.c_int(n_streams), ctypes.c_double(window), ctypes.c_double(t_lo), ctypes.c_double(t_hi),
                      ctypes.c_int(min_rx), ctypes.c_int(grid), ctypes.c_int(zero_hash), fixes.ctypes.data_as(vp), ctypes.c_int(cap),
                      ctypes.byref(nf), ms.ctypes.data_as(vp), mt.ctypes.data_as(vp), ctypes.c_int(member_cap), ctypes.byref(nm),
                      heads.ctypes.data_as(vp), ctypes.byref(nh))
    assert rc in (0, -28, -22), "a guard or the carry was overwritten (-1), or a count is out of range (-5): %d" % rc
    return rc, fixes, ms, mt, heads[:max(nh.value, 0)], nf.value, nm.value


def compare(case, fixes, ms, mt, exp, exp_ms, exp_mt, truth=None, exp_ld=None, converge=True):
    """Rows of adsb_stream_mlat (device or emulation) against the replay's: the exact fields, then the positions."""
    assert len(fixes) == len(exp), (case, len(fixes), len(exp))
    assert np.array_equal(ms, exp_ms) and mt.tobytes() == exp_mt.tobytes(), case
    for j, (f, e) in enumerate(zip(fixes, exp)):
        what = (case, j)
        assert f["ts"] == e["ts"] and f["bits"].tobytes() == e["bits"].tobytes() and f["flags"] == e["flags"], what
        assert (f["icao"], f["n_rx"], f["n_heard"], f["first"]) == (e["icao"], e["n_rx"], e["n_heard"], e["first"]), what
        if exp_ld is not None:
            own = float(np.sqrt(((exp_ld[j]["p"].astype(np.float64) - e["p"]) ** 2).sum()))
            settled = exp_ld[j]["status"] == e["status"] and abs(exp_ld[j]["iters"] - e["iters"]) <= 1 and own <= SENS
            assert settled or not converge, (what, own, exp_ld[j]["status"], e["status"])
            if not settled:                                            # the oracle's own two runs part ways: a diverging solve
                continue                                               # amplifies the last bit, and only the exact fields are compared
            if e["status"] == MR.OK:
                measured.append((case, own))
        assert f["status"] == e["status"], (what, f["status"], e["status"], f["iters"], e["iters"])
        assert abs(int(f["iters"]) - e["iters"]) <= 1, (what, f["iters"], e["iters"])
        if e["status"] != MR.OK:
            continue
        p = np.array([f["x"], f["y"], f["z"]])
        dist = float(np.sqrt(((p - e["p"]) ** 2).sum()))
        assert dist <= TOL, (what, dist)
        assert abs(f["t_tx"] - float(e["t_tx"])) <= TOL / MR.C + np.spacing(e["ts"]), what
        assert abs(f["rms_m"] - float(e["rms_m"])) <= TOL, what
        if truth is not None:
            t = np.asarray(truth[j] if isinstance(truth, list) else truth)
            own = float(np.sqrt(((e["p"] - t) ** 2).sum()))
            assert float(np.sqrt(((p - t) ** 2).sum())) <= TOL + own, (what, own)


def check(sim, case, carry, rx, truth=None, converge=True, **kw):
    """One emulated call against the replay (float64, and longdouble for the sensitivity) -> (fixes, replay rows)"""
    rc, fixes, ms, mt, heads, nf, nm = run(sim, carry, rx, **kw)
    assert rc == 0
    rk = {k: kw[k] for k in ("t_lo", "t_hi", "min_rx", "window") if k in kw}
    lst = carry.replay_list()
    exp, ems, emt = MR.mlat(lst, rk.pop("window", WINDOW), rx, **rk)
    ld = MR.mlat(lst, kw.get("window", WINDOW), rx, ft=np.longdouble, **rk)[0]
    if converge:
        assert all(e["status"] == MR.OK for e in exp), (case, [e["status"] for e in exp])      # the oracle alone converges
    t_lo, t_hi = kw.get("t_lo", -np.inf), kw.get("t_hi", np.inf)
    assert heads.tolist() == [h for h, _ in MR.groups(lst, kw.get("window", WINDOW)) if t_lo <= lst[h][0] < t_hi], case
    compare(case, fixes[:nf], ms[:nm], mt[:nm], exp, ems, emt, truth, ld, converge)
    return fixes[:nf], exp


IDENT, IDENT_LONG = reply(17, 0)


# ---- the solver ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(AIRCRAFT)))
@pytest.mark.parametrize("n_rx", [4, 5, 8])
def test_one_group_is_located(sim, k, n_rx):
    """One reply, n_rx receivers, aircraft inside and outside their hull, 1 to 12 km up: the fix is the oracle's and the truth."""
    rx = receivers(n_rx, seed=GOOD_SEED[n_rx])
    c = Carry().hear(AIRCRAFT[k], rx, range(n_rx), 0.25, IDENT, IDENT_LONG)
    fixes, exp = check(sim, "located", c, rx, truth=AIRCRAFT[k])
    assert len(fixes) == 1 and fixes["n_rx"][0] == fixes["n_heard"][0] == n_rx and fixes["status"][0] == N.MLAT_OK
    assert abs(fixes["t_tx"][0] - (T0 + 0.25)) < 1e-9 and fixes["rms_m"][0] < 1e-3


def test_all_receivers_at_one_point_is_singular(sim):
    """Four streams at one point on the x axis: the start is 10 km up the axis, every row of J is (1, 0, 0, -1) and the second
    pivot is exactly 0."""
    rx = {s: (MR.WGS_A, 0.0, 0.0) for s in range(4)}
    c = Carry()
    for s in range(4):
        c.add(T0 + 1e-4, IDENT, IDENT_LONG, s)
    fixes, exp = check(sim, "singular", c, rx, converge=False)
    assert fixes["status"].tolist() == [N.MLAT_SINGULAR] and exp[0]["status"] == MR.SINGULAR and fixes["iters"][0] == 0
    assert (fixes["x"][0], fixes["y"][0], fixes["z"][0]) == (MR.WGS_A + 10000.0, 0.0, 0.0)


def test_a_hearing_one_second_off(sim):
    """One of five arrival times is 1 s from the truth (window 2 s, so that it is still the reply's): no point fits; the oracle
    says whether that is no convergence or a large residual, and the emulation says the same."""
    rx = receivers(5, seed=GOOD_SEED[5])
    c = Carry().hear(AIRCRAFT[0], rx, range(4), 0.25, IDENT, IDENT_LONG)
    c.add(arrival(AIRCRAFT[0], rx, 4, 0.25) + 1.0, IDENT, IDENT_LONG, 4)
    fixes, exp = check(sim, "off", c, rx, converge=False, window=2.0)
    assert len(exp) == 1 and exp[0]["n_rx"] == 5
    assert exp[0]["status"] != MR.OK or float(exp[0]["rms_m"]) > 1e5      # (measured: the solve runs away and ends _SINGULAR after 2 rounds)
    assert fixes["status"][0] == exp[0]["status"]
    if exp[0]["status"] == MR.OK:
        assert fixes["rms_m"][0] > 1e5


# ---- the group rule ------------------------------------------------------------------------------------------------------------------
def fillers(n, seed):
    """n distinct long payloads that match nothing"""
    b = np.random.default_rng(seed).integers(0, 256, (n, 14)).astype(np.uint8)
    b[:, 0] = 0x8D
    b[:, 1:4] = np.array([[k >> 16, (k >> 8) & 255, k & 255] for k in range(n)], np.uint8)
    return b


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("place", [63, 255, TILE - 1, 64, 256])
def test_a_head_at_a_seam(sim, place, grid):
    """The group's head is entry `place` of the carry -- the last lane of a wavefront, the last thread of a workgroup, the last
    entry of an LDS tile (and the first of the next wavefront / workgroup) -- behind `place` foreign entries inside the window;
    its members lie on the far side.  A second hearing set of the same payload 1 ms later is no head: the first precedes it."""
    rx = RX8
    c = Carry()
    fb = fillers(place, place)
    for k in range(place):
        c.add(T0 + 0.2 + k * 1e-9, fb[k], True, 7 - k % 3)
    c.hear(AIRCRAFT[0], rx, range(6), 0.2 + 1e-5, IDENT, IDENT_LONG)
    ts = c.arrays()[0]
    assert np.argmax(ts > T0 + 0.2 + 1e-5) == place
    fixes, exp = check(sim, "seam", c, rx, truth=AIRCRAFT[0], grid=grid)
    assert fixes["n_rx"].tolist() == [6] and exp[0]["head"] == place


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("front", [TILE + 40, 2 * TILE + 9])
def test_tiles_of_foreign_entries_in_front_of_a_head(sim, front, grid):
    """More than one and more than two LDS tiles of foreign entries between the scan's start and the hearings, all inside the
    window: an equal payload `front` places in front of a would-be head is found (it is the head), across full and partial
    tiles.  The range [t_lo, t_hi) holds the hearings only, so the fillers are scanned and never solved."""
    rx = RX8
    a0 = min(arrival(AIRCRAFT[1], rx, s_, 0.3) for s_ in range(5))
    far = a0 - 1e-3
    c = Carry()
    c.add(far, IDENT, IDENT_LONG, 7)                                   # the head: one hearing, far in front
    fb = fillers(front, front)
    for k in range(front):
        c.add(a0 - 9e-4 + k * 1e-9, fb[k], True, 6)
    c.hear(AIRCRAFT[1], rx, range(5), 0.3, IDENT, IDENT_LONG)
    ts = c.arrays()[0]
    assert ts[0] == far and ts[front + 1] == a0 and ts[-1] - ts[0] <= WINDOW
    # the range holds the five only: they are no heads, entry 0 precedes them -- front + 1 places in front of the first
    rc, fixes, ms, mt, heads, nf, nm = run(sim, c, rx, t_lo=a0 - 1e-4, grid=grid)
    assert rc == 0 and nf == 0 and len(heads) == 0
    # the range holds entry 0 only: one group of six hearings whose members lie behind the fillers
    rc, fixes, ms, mt, heads, nf, nm = run(sim, c, rx, t_hi=far + 1e-5, grid=grid)
    assert rc == 0 and heads.tolist() == [0] and nf == 1 and fixes["n_rx"][0] == 6 and fixes["n_heard"][0] == 6
    # without the far hearing the first of the five is the head, `front` foreign entries behind the scan's start
    c2 = Carry()
    c2.rows = c.rows[1:]
    fixes, exp = check(sim, "tiles", c2, rx, truth=AIRCRAFT[1], t_lo=a0 - 1e-4, grid=grid)
    assert fixes["n_rx"].tolist() == [5] and exp[0]["head"] == front


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_the_cap_of_64_candidates(sim, n):
    """n hearings of one reply by n streams: the head and the first 63 others are candidates; n_heard is exact."""
    rx = receivers(n, seed=GOOD_SEED[n])
    c = Carry().hear(AIRCRAFT[0], rx, range(n), 0.4, IDENT, IDENT_LONG)
    fixes, exp = check(sim, "cap", c, rx, truth=AIRCRAFT[0])
    assert fixes["n_rx"].tolist() == [min(n, 64)] and fixes["n_heard"].tolist() == [n]


def test_a_stream_heard_twice_and_a_stream_without_a_position(sim):
    """Stream 2 hears the reply twice (only its first hearing is used); stream 5 has no position (counted in n_heard, not in
    n_rx); marker-0 entries and a foreign reply lie between the members."""
    rx = {s: p for s, p in RX8.items() if s != 5}
    c = Carry().hear(AIRCRAFT[0], RX8, [0, 1, 2, 3, 5], 0.1, IDENT, IDENT_LONG)
    late = arrival(AIRCRAFT[0], RX8, 2, 0.1) + 3e-4
    c.add(late, IDENT, IDENT_LONG, 2)
    ts = c.arrays()[0]
    for k, t in enumerate((ts[:-1] + ts[1:]) / 2):
        c.add(t, IDENT, IDENT_LONG, 6, part=False)                     # the same bytes, but the record had no PDU
        c.add(t, fillers(8, 4)[k], True, 6)
    fixes, exp = check(sim, "twice", c, rx, n_streams=8, truth=AIRCRAFT[0])
    assert fixes["n_rx"].tolist() == [4] and fixes["n_heard"].tolist() == [6]
    lst = c.replay_list()
    assert [lst[m][2] for m in exp[0]["used"]] == sorted([0, 1, 2, 3], key=lambda s: arrival(AIRCRAFT[0], RX8, s, 0.1))
    assert late not in [lst[m][0] for m in exp[0]["used"]]
    # with stream 5 positioned it is the fifth
    fixes, _ = check(sim, "twice+", c, RX8, truth=AIRCRAFT[0])
    assert fixes["n_rx"].tolist() == [5]


def test_the_chain(sim):
    """a - b - c, 1.5 ms apart with a 2 ms window: b is in a's group; c lies beyond the window from a, is no head because b
    precedes it, and is in no group.  Four receivers hear each: one fix, from a's and b's hearings."""
    rx = receivers(12, seed=5)
    c = Carry()
    for k, streams in enumerate(([0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11])):
        for s in streams:
            c.add(T0 + 0.5 + 0.0015 * k + s * 1e-7, IDENT, IDENT_LONG, s)
    fixes, exp = check(sim, "chain", c, rx, converge=False)
    assert len(fixes) == 1 and fixes["n_heard"][0] == 8 and fixes["n_rx"][0] == 8 and fixes["ts"][0] == T0 + 0.5
    assert [h for h, _ in MR.groups(c.replay_list(), WINDOW)] == [0]


def test_short_and_long_with_the_same_first_56_bits(sim):
    """A short and a long reply whose first seven bytes agree are not equal: two heads, two groups, in carry order."""
    rx = RX8
    short = IDENT.copy()
    c = Carry().hear(AIRCRAFT[0], rx, [0, 1, 2, 3], 0.1, short, False).hear(AIRCRAFT[2], rx, [4, 5, 6, 7, 0], 0.1, IDENT, True)
    fixes, exp = check(sim, "lengths", c, rx, truth=None)
    assert sorted(zip(fixes["flags"].tolist(), fixes["n_rx"].tolist())) == [(0, 4), (N.BURST_LONG, 5)]
    assert not fixes["bits"][fixes["flags"] == 0][0][7:].any()            # masked to its length
    # ... and with every hash equal only the payload words tell them apart
    f0 = run(sim, c, rx, zero_hash=1)
    assert f0[1][:f0[5]].tobytes() == fixes.tobytes()


def test_the_range_is_half_open_and_min_rx(sim):
    """t_lo / t_hi exactly on a head's ts; min_rx 4 and 5 around a group of four."""
    rx = RX8
    c = Carry().hear(AIRCRAFT[0], rx, [0, 1, 2, 3], 0.1, IDENT, IDENT_LONG).hear(AIRCRAFT[1], rx, range(6), 0.2, reply(17, 1)[0], True)
    ts = c.arrays()[0]
    h0, h1 = ts[0], ts[4]
    both, _ = check(sim, "range", c, rx, truth=[AIRCRAFT[0], AIRCRAFT[1]])
    assert both["ts"].tolist() == [h0, h1] and both["first"].tolist() == [0, 4]
    assert check(sim, "range", c, rx, t_lo=h0, t_hi=h1)[0]["ts"].tolist() == [h0]
    assert check(sim, "range", c, rx, t_lo=np.nextafter(h0, np.inf), t_hi=np.nextafter(h1, np.inf))[0]["ts"].tolist() == [h1]
    assert check(sim, "range", c, rx, t_lo=h1, t_hi=h1)[0]["ts"].tolist() == []
    assert check(sim, "range", c, rx, t_lo=h1, t_hi=h0)[0]["ts"].tolist() == []
    five, _ = check(sim, "range", c, rx, min_rx=5)
    assert five["ts"].tolist() == [h1] and five["first"].tolist() == [0] and five["n_rx"].tolist() == [6]
    assert check(sim, "range", c, rx, min_rx=7)[0]["ts"].tolist() == []
    assert run(sim, c, rx, min_rx=3)[0] == -22 and run(sim, c, rx, t_lo=np.nan)[0] == -22


def test_no_space_states_the_counts_and_writes_nothing(sim):
    rx = RX8
    c = Carry().hear(AIRCRAFT[0], rx, [0, 1, 2, 3], 0.1, IDENT, IDENT_LONG).hear(AIRCRAFT[1], rx, range(6), 0.2, reply(17, 1)[0], True)
    for cap, member_cap in ((1, 10), (2, 9), (0, 0)):
        rc, fixes, ms, mt, heads, nf, nm = run(sim, c, rx, cap=cap, member_cap=member_cap)
        assert rc == -28 and (nf, nm) == (2, 10)
        assert (fixes["first"] == -77).all() and (ms == -77).all() and (mt == -77.0).all()
    rc, fixes, ms, mt, heads, nf, nm = run(sim, c, rx, cap=2, member_cap=10)
    assert rc == 0 and (nf, nm) == (2, 10) and (fixes["first"] >= 0).all()


def test_an_empty_carry_and_a_carry_without_groups(sim):
    assert run(sim, Carry(), RX8)[5:] == (0, 0)
    c = Carry()
    for k in range(5):
        c.add(T0 + k * 0.01, IDENT, IDENT_LONG, k, part=False)
    rc, *_, heads, nf, nm = run(sim, c, RX8)
    assert rc == 0 and (len(heads), nf, nm) == (0, 0, 0)
    c = Carry().hear(AIRCRAFT[0], RX8, [0, 1, 2], 0.1, IDENT, IDENT_LONG)
    rc, *_, heads, nf, nm = run(sim, c, RX8)
    assert rc == 0 and (heads.tolist(), nf, nm) == ([0], 0, 0)


@pytest.mark.parametrize("df", [0, 4, 5, 11, 16, 17, 18, 20, 21, 24])
def test_icao(sim, df):
    """One reply of each format: DF 11/17/18 announce the address in bytes 1..3; DF 0/4/5/16/20/21 carry it under
    address/parity -- the remainder, which the host's parity helper and the oracle state --; DF 24 gives -1."""
    from oracle import adsb_oracle as O
    bits, long_ = reply(df, 7)
    syn, hdf, nbits = N.mode_s_syndrome(bits)
    par = O.mode_s_parity(np.unpackbits(bits)[None, :])
    assert hdf == df and nbits == (112 if long_ else 56) and int(par["syndrome"][0]) == syn and int(par["nbits"][0]) == nbits
    want = (int(bits[1]) << 16 | int(bits[2]) << 8 | int(bits[3])) if df in (11, 17, 18) else -1 if df == 24 else syn
    c = Carry().hear(AIRCRAFT[0], RX8, range(4), 0.1, bits, long_)
    fixes, exp = check(sim, "icao", c, RX8, truth=AIRCRAFT[0])
    assert fixes["icao"].tolist() == [want] == [exp[0]["icao"]]


# ---- random fleets ---------------------------------------------------------------------------------------------------------
@st.composite
def fleets(draw):
    """4 .. 9 receivers, some without a position; replies 5 ms apart out of a pool of six payloads, each heard by a subset of
    the receivers at its true arrival time (sometimes twice by one stream, sometimes as a record without a PDU)."""
    n_streams = draw(st.integers(4, 9))
    unset = draw(st.sets(st.integers(0, n_streams - 1), max_size=2))
    replies = draw(st.lists(st.tuples(st.integers(0, 5), st.integers(0, len(AIRCRAFT) - 1),
                                      st.lists(st.tuples(st.integers(0, n_streams - 1), st.integers(0, 9)), min_size=1, max_size=12)),
                            min_size=1, max_size=25))
    seed = draw(st.integers(0, 2 ** 16))
    bounds = draw(st.tuples(st.floats(0.0, 0.2), st.floats(0.0, 0.2)))
    min_rx = draw(st.integers(4, 6))
    grid = draw(st.integers(0, 3))
    return n_streams, unset, replies, seed, bounds, min_rx, grid


@settings(max_examples=20, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
@given(fleets())
def test_random_fleets(sim, world):
    """Property: emulation = replay -- heads, members, every exact field, positions within TOL -- for random fleets and carries."""
    n_streams, unset, replies, seed, bounds, min_rx, grid = world
    rx_all = receivers(n_streams, seed=seed)
    rx = {s: p for s, p in rx_all.items() if s not in unset}
    pool = [reply(df, k) for k, df in enumerate((17, 17, 11, 4, 20, 0))]
    c = Carry()
    for k, (which, plane, hear) in enumerate(replies):
        bits, long_ = pool[which]
        for s, kind in hear:
            t = arrival(AIRCRAFT[plane], rx_all, s, 0.005 * k)
            c.add(t, bits, long_, s, part=kind != 0)
            if kind == 1:
                c.add(t + 1e-5, bits, long_, s)                        # the same stream again
    lo, hi = T0 + min(bounds), T0 + max(bounds)
    check(sim, "random", c, rx, n_streams=n_streams, converge=False, min_rx=min_rx, grid=grid)
    check(sim, "random", c, rx, n_streams=n_streams, converge=False, t_lo=lo, t_hi=hi, min_rx=4, grid=grid)


# ---- the periodic carry: the compaction's scan beyond 256 chunks, the kernels' second grid-stride round -------------------
# One period of PERIOD = 65 entries (coprime to 64, 256 and 1024: heads and members drift over every lane, workgroup place and
# tile place), all within 1 ms, repeated every SPACING = 2^-7 s from EPOCH = 1024 s on, with the same payloads in every period
# -- a kernel that matched across periods would show.  Every timestamp in [1024, 2048) is a multiple of 2^-42 s, so adding
# k * 2^-7 is exact and the solver's inputs (differences of arrival times) of period k are bit for bit period 0's.
EPOCH, SPACING, PERIOD = 1024.0, 2.0 ** -7, 65
SHORT4 = reply(4, 1)[0]                                   # a short reply whose address lies under address/parity


def period0():
    """-> Carry: a long reply of AIRCRAFT[0] heard by streams 0 .. 5, and once more by stream 2; a short reply of AIRCRAFT[1]
    heard by streams 0 .. 4; a reply heard by three streams (no fix); a marker-0 entry with the long reply's bytes; 49 fillers."""
    at = lambda p, s: EPOCH + float(np.sqrt(((np.asarray(p) - np.asarray(RX8[s])) ** 2).sum())) / MR.C      # noqa: E731
    c = Carry()
    for s in range(6):
        c.add(at(AIRCRAFT[0], s), IDENT, IDENT_LONG, s)
    c.add(at(AIRCRAFT[0], 2) + 1e-4, IDENT, IDENT_LONG, 2)
    c.add(at(AIRCRAFT[0], 3) + 1e-6, IDENT, IDENT_LONG, 6, part=False)
    for s in range(5):
        c.add(at(AIRCRAFT[1], s), SHORT4, False, s)
    three = reply(17, 2)[0]
    for s in (5, 6, 7):
        c.add(EPOCH + 2.003e-4 + s * 1e-6, three, True, s)
    fb = fillers(PERIOD - len(c.rows), 65)
    for k in range(len(fb)):
        c.add(EPOCH + 1e-5 + k * 1.3e-5, fb[k], True, 7 - k % 3)
    ts = c.arrays()[0]
    assert len(ts) == PERIOD and (np.diff(ts) > 0).all() and EPOCH < ts[0] and ts[-1] - ts[0] < 1e-3
    assert SPACING - (ts[-1] - ts[0]) > WINDOW                         # no entry of another period is within the window
    return c


def periodic(n):
    """-> (ts, bits, marker, stream) of the first n entries of the periodic carry, and period 0's arrays"""
    p0 = period0().arrays()
    k = -(-n // PERIOD)
    shift = np.arange(k) * SPACING
    ts = (p0[0][None, :] + shift[:, None]).ravel()[:n]
    whole = n // PERIOD
    assert ts[-1] < 2 * EPOCH and (ts[:whole * PERIOD].reshape(whole, PERIOD) - shift[:whole, None] == p0[0]).all()      # the shift is exact
    return (ts, np.tile(p0[1], (k, 1))[:n].copy(), np.tile(p0[2], k)[:n].copy(), np.tile(p0[3], k)[:n].copy()), p0


def replay_rows(p0, k, n=PERIOD):
    """the first n entries of period k, as MR.mlat takes them"""
    return [(float(p0[0][i] + k * SPACING), None if p0[2][i] == 0 else MR.payload_of(p0[1][i], p0[2][i] == 2), int(p0[3][i])) for i in range(n)]


def check_periodic(sim, case, n):
    """One call over the first n entries of the periodic carry -> (fixes, member_stream, member_ts, heads, period 0's arrays, fixes per period, members per period).
    Period 0 alone against the replay (check()); every whole period k against period 0's rows of THIS call: the exact fields
    equal, `first` + members-per-period * k, ts and member_ts + k * SPACING exactly, x / y / z / rms_m bit for bit, t_tx within
    one spacing of the shifted value; the first, the last and (where there is one) the period holding entry 524 288 against a
    replay of their own entries; the cut period, if any, against the replay of its entries."""
    arrays, p0 = periodic(n)
    c0 = period0()
    lst0 = c0.replay_list()
    assert lst0 == replay_rows(p0, 0)
    truth = [AIRCRAFT[0] if e["flags"] else AIRCRAFT[1] for e in MR.mlat(lst0, WINDOW, RX8)[0]]
    alone, exp0 = check(sim, case, c0, RX8, truth=truth)               # asserts status == OK of the oracle
    heads0 = [h for h, _ in MR.groups(lst0, WINDOW)]
    per_f, per_m, per_h = len(exp0), sum(e["n_rx"] for e in exp0), len(heads0)
    assert (per_f, per_m) == (2, 11) and sorted(alone["n_heard"].tolist()) == [5, 7]

    rc, fixes, ms, mt, heads, nf, nm = run_arrays(sim, *arrays, RX8)
    assert rc == 0
    fixes, ms, mt = fixes[:nf], ms[:nm], mt[:nm]
    whole, cut = divmod(n, PERIOD)
    cut_exp = MR.mlat(replay_rows(p0, whole, cut), WINDOW, RX8) if cut else ([], np.zeros(0, np.int32), np.zeros(0))
    cut_heads = [h for h, _ in MR.groups(replay_rows(p0, whole, cut), WINDOW)] if cut else []
    assert (nf, nm, len(heads)) == (whole * per_f + len(cut_exp[0]), whole * per_m + len(cut_exp[1]), whole * per_h + len(cut_heads)), case
    ks = np.arange(whole)
    assert np.array_equal(heads[:whole * per_h].reshape(whole, per_h), np.array(heads0)[None, :] + PERIOD * ks[:, None]), case
    assert heads[whole * per_h:].tolist() == [whole * PERIOD + h for h in cut_heads], case

    F = fixes[:whole * per_f].reshape(whole, per_f)
    assert F[0].tobytes() == alone.tobytes(), case                     # the carry behind period 0 changes nothing of its rows
    for name in ("bits", "flags", "icao", "n_rx", "n_heard", "status", "iters"):
        assert (F[name] == F[0][name][None]).all(), (case, name)
    assert np.array_equal(F["first"], F[0]["first"][None, :] + per_m * ks[:, None]), case
    assert np.array_equal(F["ts"], F[0]["ts"][None, :] + SPACING * ks[:, None]), case
    M_s, M_t = ms[:whole * per_m].reshape(whole, per_m), mt[:whole * per_m].reshape(whole, per_m)
    assert (M_s == M_s[0][None, :]).all() and np.array_equal(M_t, M_t[0][None, :] + SPACING * ks[:, None]), case
    for name in ("x", "y", "z", "rms_m"):
        assert np.array_equal(F[name].view(np.uint64), np.broadcast_to(F[0][name].view(np.uint64)[None, :], F[name].shape)), (case, name)
    shifted = F[0]["t_tx"][None, :] + SPACING * ks[:, None]
    assert (np.abs(F["t_tx"] - shifted) <= np.spacing(shifted)).all(), case

    for k in sorted({0, whole - 1} | ({524288 // PERIOD} if n > 524288 + PERIOD else set())):
        rows = F[k].copy()
        rows["first"] -= per_m * k
        compare((case, k), rows, M_s[k], M_t[k], *MR.mlat(replay_rows(p0, k), WINDOW, RX8), truth=truth)
    if cut:
        rows = fixes[whole * per_f:].copy()
        rows["first"] -= per_m * whole
        compare((case, "cut"), rows, ms[whole * per_m:], mt[whole * per_m:], *cut_exp, converge=False)
    return fixes, ms, mt, heads, p0, per_f, per_m


N_SCAN = 256 * 256 + 257          # 258 chunks: k_mlat_scan's threads take two each, thread 128 the last, threads 129 .. 255 none


def test_the_scan_with_more_than_256_chunks(sim):
    """k_mlat_scan with per = 2: a range of 65 793 entries, the smallest that reaches the path (1 012 periods and 13 entries of
    the next).  The emulator takes 8 s for it (measured where this was written); the device runs the same test in tests/test_gpu_mlat_device.py."""
    fixes, ms, mt, heads, *_ = check_periodic(sim, "scan", N_SCAN)
    assert (N_SCAN + 255) // 256 == 258 and len(fixes) >= 2 * (N_SCAN // PERIOD)


def carry_words_numpy(ts, bits, mk, stream, zero_hash=0):
    """The carry's words in NumPy, as tests/sim/mlat_driver.cpp's make_carry states them -- only for a machine where the emulator
    library cannot be built; test_the_carry_words_in_numpy holds them equal to the emulator's."""
    n = len(ts)
    b16 = np.zeros((n, 16), np.uint8)
    b16[:, :14] = bits
    w = b16.view("<u8").reshape(n, 2)
    mk64 = mk.astype(np.uint64)
    a = np.where(mk == 0, np.uint64(0), np.where(mk == 2, w[:, 0], w[:, 0] & np.uint64(0x00FFFFFFFFFFFFFF)))
    b = np.where(mk == 2, w[:, 1], np.uint64(0))
    with np.errstate(over="ignore"):
        k = a ^ (b * np.uint64(0x9E3779B97F4A7C15))
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    h = np.uint64(0) if zero_hash else (k & np.uint64(0xFFFFFFFF))
    out = np.zeros((n, 4), np.uint64)
    out[:, 0] = np.asarray(ts, np.float64).view(np.uint64)
    out[:, 1], out[:, 2] = a, b
    out[:, 3] = h | ((stream.astype(np.uint64) & np.uint64(0xFFFFFF)) << np.uint64(32)) | (mk64 << np.uint64(56))
    return out


def emulator_words(sim, ts, bits, mk, stream, zero_hash=0):
    """-> [n, 4] uint64: sim_mlat_carry's words"""
    out = np.zeros((len(ts), 4), np.uint64)
    ts, bits, mk, stream = (np.ascontiguousarray(x) for x in (ts, bits, mk, stream))
    sim.sim_mlat_carry(ts.ctypes.data_as(vp), bits.ctypes.data_as(vp), mk.ctypes.data_as(vp), stream.ctypes.data_as(vp), ctypes.c_int(len(ts)),
                       ctypes.c_int(zero_hash), out.ctypes.data_as(vp))
    return out


def test_the_carry_words_in_numpy(sim):
    """carry_words_numpy = the emulator driver's words: the period (long, short, marker 0) and random bytes, markers and streams"""
    rng = np.random.default_rng(5)
    n = 500
    rand = (EPOCH + np.sort(rng.uniform(0, 1, n)), rng.integers(0, 256, (n, 14)).astype(np.uint8), rng.integers(0, 3, n).astype(np.int32),
            rng.integers(0, 2 ** 24, n).astype(np.int32))
    for arrays in (period0().arrays(), rand):
        for zero_hash in (0, 1):
            assert emulator_words(sim, *arrays, zero_hash).tobytes() == carry_words_numpy(*arrays, zero_hash).tobytes()


def test_the_oracles_own_sensitivity():
    """Runs last in this file: the largest float64-vs-longdouble distance of the oracle over the cases compared above is what
    the module's docstring states, and TOL follows from it."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("this platform's long double is a double: the sensitivity was measured where it is wider")
    assert measured, "the cases above ran"
    worst = max(measured, key=lambda m: m[1])
    print("oracle float64 vs longdouble: worst %.3g m in case %r over %d fixes; TOL %.3g m" % (worst[1], worst[0], len(measured), TOL))
    assert worst[1] <= SENS and TOL == 2e-3


# ---- the host-rule helpers -----------------------------------------------------------------------------------------------------
def test_geodetic_round_trip():
    """adsb_geodetic_to_ecef / adsb_ecef_to_geodetic at the poles, the equator, the date line and -500 .. 20000 m, against the
    longdouble evaluation of the same formulas: forward within 16 x the float64 evaluation's own distance from it (never less
    than 2 nm, a few ulps of the radius), the round trip within the same in position."""
    N.load()
    worst = 0.0
    for lat in (-90.0, -89.999, -45.0, -1e-9, 0.0, 33.3, 52.0, 89.999, 90.0):
        for lon in (-180.0, -179.999999, -90.0, 0.0, 5.0, 179.999999, 180.0):
            for alt in (-500.0, 0.0, 11000.0, 20000.0):
                ld = MR.geodetic_to_ecef(lat, lon, alt, np.longdouble)
                own = float(np.sqrt(((MR.geodetic_to_ecef(lat, lon, alt) - ld) ** 2).sum()))
                tol = max(16 * own, 2e-9)
                p = np.array(N.geodetic_to_ecef(lat, lon, alt))
                assert float(np.sqrt(((p - ld.astype(np.float64)) ** 2).sum())) <= tol, (lat, lon, alt)
                la, lo, al = N.ecef_to_geodetic(*p)
                back = MR.geodetic_to_ecef(la, lo, al, np.longdouble)
                d = float(np.sqrt(((back - ld) ** 2).sum()))
                worst = max(worst, d)
                assert d <= 2 * tol + 1e-8, (lat, lon, alt, d)
                assert abs(la - lat) < 1e-9 and abs(al - alt) < 1e-8, (lat, lon, alt, la, al)
                if abs(lat) < 90:                                      # (at a pole every longitude is the same point)
                    assert abs((lo - lon + 180.0) % 360.0 - 180.0) < 1e-9
    print("geodetic round trip: worst %.3g m" % worst)


# ---- build facts -----------------------------------------------------------------------------------------------------------
KERNELS = ["k_mlat_count", "k_mlat_groups", "k_mlat_heads", "k_mlat_place", "k_mlat_range", "k_mlat_scan", "k_mlat_solve"]


def test_kernel_resources_mlat(sim):
    """The fourth translation unit's report: exactly the k_mlat_* kernels, none with scratch or spills, LDS as DESIGN.md §3i
    states; the other three units keep their sources and their kernel sets."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES_MLAT))
    name = lambda k: re.search(r"k_mlat_[a-z_]+?(?=E)", k).group(0)      # noqa: E731
    assert sorted(name(k) for k in res) == KERNELS, sorted(res)
    for k, v in res.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    lds = {name(k): v["lds_bytes_per_block"] for k, v in res.items()}
    assert lds["k_mlat_heads"] == TILE * 16 + 8 == sim.sim_mlat_lds_bytes(0)
    assert lds["k_mlat_count"] == lds["k_mlat_place"] == 32 == sim.sim_mlat_lds_bytes(1)
    assert lds["k_mlat_scan"] == 2048 == sim.sim_mlat_lds_bytes(2)
    assert lds["k_mlat_range"] == lds["k_mlat_groups"] == lds["k_mlat_solve"] == 0
    design = open(os.path.join(HERE, "..", "DESIGN.md")).read()
    assert "### 3i." in design and "%d bytes of LDS" % (TILE * 16 + 8) in design
    dedup, shared, main = json.load(open(B.RES_DEDUP)), json.load(open(B.RES_SHARED)), json.load(open(B.RES))
    assert len(dedup) == 4 and all("k_dedup_" in k for k in dedup)
    assert len(shared) == 6 and all("k_shared_" in k for k in shared)
    assert not any("k_mlat" in k for k in list(main) + list(shared) + list(dedup))
    gold = json.load(open(os.path.join(HERE, "golden", "merge_parent_kernels.json")))
    assert sorted(gold) == sorted(k for k in main if "k_merge_" not in k) and len(main) == len(gold) + 3
    assert B.SOURCES == ["adsb_hip.hip"] and B.SHARED_SOURCE == "adsb_shared.hip" and B.DEDUP_SOURCE == "adsb_dedup.hip"
    assert B.MLAT_SOURCE == "adsb_mlat.hip" and all(d in B.DEPS for d in ("adsb_mlat.hip", "adsb_mlat.h", "adsb_mlat_device.h"))


def test_the_sizing_rule(sim):
    """adsb_mlat.h's layout(): every part on a 256-byte boundary, room for nc heads, nc / 4 + 1 fixes and nc members."""
    for nc, ns in ((1, 1), (255, 3), (256, 8), (257, 8), (100000, 64)):
        chunks = (nc + 255) // 256 + 1
        parts = [16, 16, 16, nc * 4, chunks * 4, chunks * 4, nc * 4, nc * 4, nc * 4, nc * 4, ns * 24, (nc // 4 + 1) * 88, nc * 4, nc * 8]
        assert sim.sim_mlat_layout_bytes(nc, ns) == sum((p + 255) // 256 * 256 for p in parts)


def test_constants_and_export_names():
    hdr = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_ABI_VERSION (\d+)", hdr).group(1) == "5" and N.ABI_VERSION == 5
    assert float(re.search(r"#define ADSB_MLAT_C ([0-9.]+)", hdr).group(1)) == N.MLAT_C == MR.C == 299702547.0
    assert abs(299792458.0 / 1.0003 - N.MLAT_C) < 1.0
    for k, name in enumerate(("OK", "NO_CONVERGE", "SINGULAR")):
        assert re.search(r"#define ADSB_MLAT_%s (\d+)" % name, hdr).group(1) == str(getattr(N, "MLAT_" + name)) == str(k)
    assert (MR.OK, MR.NO_CONVERGE, MR.SINGULAR) == (N.MLAT_OK, N.MLAT_NO_CONVERGE, N.MLAT_SINGULAR)
    for name in ("adsb_stream_set_ecef", "adsb_stream_mlat", "adsb_stream_mlat_stats"):
        assert name in N.EXPORTS and re.search(r"^int %s\(adsb_ctx\* ctx" % name, hdr, re.M)
    for name in ("adsb_geodetic_to_ecef", "adsb_ecef_to_geodetic"):
        assert name in N.EXPORTS and re.search(r"^void %s\(double" % name, hdr, re.M)
    for name in ("set_stream_ecef", "stream_mlat", "stream_mlat_stats"):
        assert callable(getattr(N.Context, name))
    assert callable(N.geodetic_to_ecef) and callable(N.ecef_to_geodetic)
    assert [f for f in N.MLAT_DTYPE.names] == ["ts", "x", "y", "z", "t_tx", "rms_m", "bits", "flags", "icao", "n_rx", "n_heard", "status",
                                               "iters", "first"]
    fields = re.search(r"typedef struct adsb_mlat_fix \{(.*?)\} adsb_mlat_fix;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)(?:\[14\])?[,;]", fields) == ["ts", "x", "y", "z", "t_tx", "rms_m", "bits", "flags", "icao", "n_rx", "n_heard", "status",
                                                            "iters", "first"]
