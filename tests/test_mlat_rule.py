"""adsb_stream_mlat_rule on the CPU: the emulated kernels of gr_adsb_amd/csrc/adsb_mlat_rule_device.h (tests/sim/mlat_rule_driver.cpp:
the launches in adsb_hip.hip's order, the host's argument table, sizing and -ENOSPC rules restated, guard bytes behind every
part) against the plain-Python restatement of the header's DAMPED RULE in tests/mlat_rule_replay.py.  The worlds, the carries
and the group rule's oracle are tests/test_mlat.py's and tests/mlat_replay.py's.

Exact: the heads, the member lists, n_rx, n_heard, bits, flags, icao, status, iters, first, alt_ft, tries and the aux flags.
Within TOL of the float64 replay: x / y / z, rms_m, up_m; t_tx within TOL / C and one spacing; lambda to 1e-9 of itself (it is a
power of ten walked up and down by the same decisions).  Where the replay's own float64 and np.longdouble runs part ways in
status, tries, iters or the aux flags -- a decision S' <= S taken at rounding level -- only the group's exact fields are
compared; no case meant to converge may be one of those (compare() asserts it).

TOL.  The float64 replay against its np.longdouble run over every converging fix compared in this file differs by at most
SENS = 5e-7 m (measured: 5.3e-8 m over 81 fixes, the worst a four-receiver fix below the receivers' plane;
test_the_replays_own_sensitivity prints and bounds it); the device sums the hearings in another order, so 16 x SENS is allowed,
and never less than 2e-3 m, twice the stopping threshold: TOL = max(16 x SENS, 2e-3) = 2e-3 m.

What a green run here does not cover: the host's own code and the Python surface (tests/test_gpu_mlat_rule.py), and what hipcc
makes of the kernels, the real launchers' cover() and the second grid-stride round (tests/test_gpu_mlat_rule_device.py runs
this file's cases on the MI355X and compares the device's bytes with this emulation's)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import decode_replay as DR
import mlat_replay as MR
import mlat_rule_replay as RR
import test_mlat as TM
from gr_adsb_amd import _native as N
from test_mlat import AIRCRAFT, RX8, T0, WINDOW, Carry, receivers, reply

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
RULE_SO = os.path.join(SIM_DIR, "libadsb_mlat_rule_sim.so")
SENS = 5e-7
TOL = max(16 * SENS, 2e-3)
GN, LM, RESTART, ALTITUDE = RR.SOLVER_GN, RR.SOLVER_LM, RR.RESTART, RR.ALTITUDE
vp = ctypes.c_void_p
measured = []                 # (case, float64-vs-longdouble distance) of every converged fix compared in this run


def rule_lib():
    csrc = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, f) for f in ("mlat_rule_driver.cpp", "mlat_driver.cpp", "hipsim.h", "mlat_host_rule.h", "mlat_rule_host_rule.h")] + \
        [os.path.join(csrc, f) for f in ("adsb_mlat_device.h", "adsb_mlat.h", "adsb_dedup_device.h", "adsb_mlat_rule_device.h", "adsb_mlat_rule.h")]
    if not (os.path.exists(RULE_SO) and all(os.path.getmtime(RULE_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", RULE_SO])
    lib = ctypes.CDLL(RULE_SO)
    for f in (lib.sim_mlat_layout_bytes, lib.sim_mlat_rule_layout_bytes):
        f.restype = ctypes.c_ulonglong
        f.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = rule_lib()
    assert lib.sim_mlat_fix_bytes() == N.MLAT_DTYPE.itemsize == 88 and lib.sim_mlat_aux_bytes() == N.MLAT_AUX_DTYPE.itemsize == 32
    return lib


# ---- payloads with an altitude -----------------------------------------------------------------------------------------------
def set_field(b, lo, n, v):
    for k in range(n):
        i = lo + k
        bit = (v >> (n - 1 - k)) & 1
        b[i >> 3] = (int(b[i >> 3]) & ~(0x80 >> (i & 7))) | (bit << (7 - (i & 7)))


def ac13_of(alt_ft, q=1, m=0):
    n = (alt_ft + 1000) // 25
    return ((n >> 5) << 7) | (m << 6) | (((n >> 4) & 1) << 5) | (q << 4) | (n & 0xF)


def ac12_of(alt_ft, q=1):
    n = (alt_ft + 1000) // 25
    return ((n >> 4) << 5) | (q << 4) | (n & 0xF)


def alt_reply(df, alt_ft, seed=0, tc=11, q=1, m=0, raw=None):
    """A reply of format df announcing alt_ft: DF 0 / 4 / 16 / 20 in bits 19..31, DF 17 (type code tc) in bits 40..51; raw: the
    field's value as it stands"""
    b, long_ = reply(df, 50 + seed)
    if df == 17:
        set_field(b, 32, 5, tc)
        set_field(b, 40, 12, ac12_of(alt_ft, q) if raw is None else raw)
    else:
        set_field(b, 19, 13, ac13_of(alt_ft, q, m) if raw is None else raw)
    return b, long_


def at_height(lat, lon, alt_ft):
    return MR.geodetic_to_ecef(lat, lon, 0.3048 * alt_ft)


# aircraft whose height is exactly what a 25 ft altitude code says
ALT_FT = [29525, 3275]
AIDED = [at_height(52.2, 4.7, ALT_FT[0]), at_height(51.6, 5.9, ALT_FT[1])]
RX3 = receivers(3, seed=4)        # three receivers from which the REPLAY's aided run ends on both AIDED aircraft (found on the CPU)


# ---- one call ----------------------------------------------------------------------------------------------------------------
def run_rule(sim, carry, rx, **kw):
    return run_rule_arrays(sim, *carry.arrays(), rx, **kw)


def run_rule_arrays(sim, ts, bits, mk, stream, rx, solver=LM, flags=RESTART, min_rx=4, reserved=0, alt_weight=1.0, n_streams=None, t_lo=-np.inf,
                    t_hi=np.inf, grid=0, zero_hash=0, cap=None, member_cap=None, window=WINDOW, want_aux=True):
    """-> (rc, fixes, aux, member_stream, member_ts, heads, n_fixes, n_members)"""
    nc = len(ts)
    n_streams = n_streams or (max([int(stream.max()) if nc else 0] + list(rx)) + 1)
    rxa = TM.rx_array(rx, n_streams)
    cap = nc // 3 + 1 if cap is None else cap
    member_cap = nc if member_cap is None else member_cap
    fixes, aux = np.zeros(cap, dtype=N.MLAT_DTYPE), np.zeros(cap, dtype=N.MLAT_AUX_DTYPE)
    fixes["first"] = -77
    aux["tries"] = -77
    ms, mt = np.full(member_cap, -77, np.int32), np.full(member_cap, -77.0, np.float64)
    heads = np.zeros(max(nc, 1), np.int32)
    nf, nm, nh = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = sim.sim_mlat_rule(ts.ctypes.data_as(vp), bits.ctypes.data_as(vp), mk.ctypes.data_as(vp), stream.ctypes.data_as(vp), ctypes.c_int(nc),
                           rxa.ctypes.data_as(vp), ctypes.c_int(n_streams), ctypes.c_double(window), ctypes.c_double(t_lo), ctypes.c_double(t_hi),
                           ctypes.c_int(solver), ctypes.c_int(flags), ctypes.c_int(min_rx), ctypes.c_int(reserved), ctypes.c_double(alt_weight),
                           ctypes.c_int(grid), ctypes.c_int(zero_hash), fixes.ctypes.data_as(vp), aux.ctypes.data_as(vp) if want_aux else vp(None),
                           ctypes.c_int(cap), ctypes.byref(nf), ms.ctypes.data_as(vp), mt.ctypes.data_as(vp), ctypes.c_int(member_cap),
                           ctypes.byref(nm), heads.ctypes.data_as(vp), ctypes.byref(nh))
    assert rc in (0, -28, -22), "a guard or the carry was overwritten (-1), or a count is out of range (-5): %d" % rc
    return rc, fixes, aux, ms, mt, heads[:max(nh.value, 0)], nf.value, nm.value


def decisions(e):
    return e["status"], e["tries"], e["iters"], e["aux_flags"]


def compare(case, fixes, aux, ms, mt, exp, exp_ms, exp_mt, truth=None, exp_ld=None, converge=True):
    """Rows of adsb_stream_mlat_rule (device or emulation) against the replay's"""
    assert len(fixes) == len(aux) == len(exp), (case, len(fixes), len(exp))
    assert np.array_equal(ms, exp_ms) and mt.tobytes() == exp_mt.tobytes(), case
    for j, (f, a, e) in enumerate(zip(fixes, aux, exp)):
        what = (case, j)
        assert f["ts"] == e["ts"] and f["bits"].tobytes() == e["bits"].tobytes() and f["flags"] == e["flags"], what
        assert (f["icao"], f["n_rx"], f["n_heard"], f["first"]) == (e["icao"], e["n_rx"], e["n_heard"], e["first"]), what
        assert a["alt_ft"] == e["alt_ft"] and a["reserved"] == 0 and bool(a["flags"] & RR.AUX_AIDED) == (e["alt_ft"] != -1), what
        if exp_ld is not None:
            own = float(np.sqrt(((exp_ld[j]["p"].astype(np.float64) - e["p"]) ** 2).sum()))
            settled = decisions(exp_ld[j]) == decisions(e) and (e["status"] != RR.OK or own <= SENS)
            assert settled or not converge, (what, own, decisions(exp_ld[j]), decisions(e))
            if not settled:
                continue
            if e["status"] == RR.OK:
                measured.append((case, own))
        assert (f["status"], a["tries"], f["iters"], a["flags"]) == decisions(e), (what, (f["status"], a["tries"], f["iters"], a["flags"]), decisions(e))
        assert abs(a["lambda"] - float(e["lam"])) <= 1e-9 * float(e["lam"]), (what, a["lambda"], e["lam"])
        if e["status"] != RR.OK:
            continue
        p = np.array([f["x"], f["y"], f["z"]])
        dist = float(np.sqrt(((p - e["p"]) ** 2).sum()))
        assert dist <= TOL, (what, dist)
        assert abs(f["t_tx"] - float(e["t_tx"])) <= TOL / MR.C + np.spacing(e["ts"]), what
        assert abs(f["rms_m"] - float(e["rms_m"])) <= TOL and abs(a["up_m"] - float(e["up_m"])) <= TOL, what
        if truth is not None:
            t = np.asarray(truth[j] if isinstance(truth, list) else truth)
            own = float(np.sqrt(((e["p"] - t) ** 2).sum()))
            assert float(np.sqrt(((p - t) ** 2).sum())) <= TOL + own, (what, own)


def check(sim, case, carry, rx, truth=None, converge=True, **kw):
    """One emulated call against the replay (float64, and longdouble for the sensitivity) -> (fixes, aux, replay rows)"""
    rc, fixes, aux, ms, mt, heads, nf, nm = run_rule(sim, carry, rx, **kw)
    assert rc == 0
    rk = {k: kw[k] for k in ("t_lo", "t_hi", "min_rx", "flags", "alt_weight") if k in kw}
    lst, window = carry.replay_list(), kw.get("window", WINDOW)
    exp, ems, emt = RR.mlat(lst, window, rx, **rk)
    ld = RR.mlat(lst, window, rx, ft=np.longdouble, **rk)[0]
    if converge:
        assert all(e["status"] == RR.OK for e in exp), (case, [e["status"] for e in exp])
    t_lo, t_hi = kw.get("t_lo", -np.inf), kw.get("t_hi", np.inf)
    assert heads.tolist() == [h for h, _ in MR.groups(lst, window) if t_lo <= lst[h][0] < t_hi], case
    compare(case, fixes[:nf], aux[:nf], ms[:nm], mt[:nm], exp, ems, emt, truth, ld, converge)
    return fixes[:nf], aux[:nf], exp


IDENT, IDENT_LONG = TM.IDENT, TM.IDENT_LONG


# ---- _GN is adsb_stream_mlat ---------------------------------------------------------------------------------------------------
def gn_worlds():
    yield "located", Carry().hear(AIRCRAFT[2], receivers(5, seed=TM.GOOD_SEED[5]), range(5), 0.25, IDENT, IDENT_LONG), receivers(5, seed=TM.GOOD_SEED[5]), {}
    two = Carry().hear(AIRCRAFT[0], RX8, [0, 1, 2, 3], 0.1, IDENT, IDENT_LONG).hear(AIRCRAFT[1], RX8, range(6), 0.2, reply(17, 1)[0], True)
    yield "range", two, RX8, {}
    yield "min_rx", two, RX8, dict(min_rx=5)
    yield "no space", two, RX8, dict(cap=1, member_cap=10)
    yield "count query", two, RX8, dict(cap=0, member_cap=0)
    yield "period", TM.period0(), RX8, {}
    yield "singular", Carry().hear((MR.WGS_A, 0.0, 0.0), {s: (MR.WGS_A, 0.0, 0.0) for s in range(4)}, range(4), 0.1, IDENT, IDENT_LONG), \
        {s: (MR.WGS_A, 0.0, 0.0) for s in range(4)}, {}


def test_gauss_newton_through_the_rule_is_adsb_stream_mlat(sim):
    """{_GN, 0, m >= 4}: the fixes, the member lists, the heads, the counts and the return code of sim_mlat, byte for byte, on
    test_mlat.py's worlds; the aux rows say alt_ft -1 and nothing else."""
    for case, carry, rx, kw in gn_worlds():
        want = TM.run(sim, carry, rx, **kw)
        cap = kw.get("cap", len(carry.rows) // 4 + 1)
        rc, fixes, aux, ms, mt, heads, nf, nm = run_rule(sim, carry, rx, solver=GN, flags=0, **dict(kw, cap=cap))
        assert (rc, nf, nm) == (want[0], want[5], want[6]) and np.array_equal(heads, want[4]), case
        assert fixes.tobytes() == want[1].tobytes() and ms.tobytes() == want[2].tobytes() and mt.tobytes() == want[3].tobytes(), case
        if rc == 0:
            assert (aux["alt_ft"][:nf] == -1).all() and all((aux[name][:nf] == 0).all() for name in ("up_m", "lambda", "tries", "flags", "reserved")), case
        assert (aux["tries"][nf if rc == 0 else 0:] == -77).all(), case


# ---- the damped solver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(AIRCRAFT)))
@pytest.mark.parametrize("n_rx", [4, 5, 8])
def test_one_group_is_located(sim, k, n_rx):
    """test_mlat.py's geometries, at which the undamped rule converges: the damped one ends on the truth too."""
    rx = receivers(n_rx, seed=TM.GOOD_SEED[n_rx])
    c = Carry().hear(AIRCRAFT[k], rx, range(n_rx), 0.25, IDENT, IDENT_LONG)
    fixes, aux, exp = check(sim, "located", c, rx, truth=AIRCRAFT[k])
    assert len(fixes) == 1 and fixes["n_rx"][0] == fixes["n_heard"][0] == n_rx and fixes["status"][0] == N.MLAT_OK
    assert abs(fixes["t_tx"][0] - (T0 + 0.25)) < 1e-9 and fixes["rms_m"][0] < 1e-3 and aux["alt_ft"][0] == -1
    # (AIRCRAFT[1], 1000 m up, really is below the receivers' centroid plane: the restart tries its mirror image and keeps the truth)
    assert (aux["up_m"][0] > 0) == (k != 1) and bool(aux["flags"][0] & RR.AUX_SECOND_KEPT) is False


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65])
def test_the_number_of_hearings(sim, n):
    """n hearings by n streams: the head and the first 63 others are candidates, as for the undamped rule"""
    rx = receivers(n, seed=TM.GOOD_SEED[n])
    c = Carry().hear(AIRCRAFT[0], rx, range(n), 0.4, IDENT, IDENT_LONG)
    fixes, aux, exp = check(sim, "hearings", c, rx, truth=AIRCRAFT[0])
    assert fixes["n_rx"].tolist() == [min(n, 64)] and fixes["n_heard"].tolist() == [n]


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("n", [3, 4, 5])
def test_aided_groups(sim, k, n):
    """The reply's own altitude as one more row: three receivers are enough, and four or five take it too; no restart."""
    rx = RX3 if n == 3 else receivers(n, seed=TM.GOOD_SEED[n])
    bits, long_ = alt_reply(17, ALT_FT[k], tc=11)
    c = Carry().hear(AIDED[k], rx, range(n), 0.25, bits, long_)
    fixes, aux, exp = check(sim, "aided", c, rx, truth=AIDED[k], flags=RESTART | ALTITUDE, min_rx=3)
    assert fixes["n_rx"].tolist() == [n] and aux["alt_ft"].tolist() == [ALT_FT[k]] and aux["flags"].tolist() == [RR.AUX_AIDED]
    assert float(np.sqrt(((exp[0]["p"] - AIDED[k]) ** 2).sum())) < 0.01      # the truth: the aircraft is at the coded height
    # a weight is the caller's: the row still holds, the fix is the replay's
    check(sim, "aided w", c, rx, truth=AIDED[k], flags=ALTITUDE, min_rx=3, alt_weight=0.25)


def three_and_four():
    """A three-hearing group with an altitude, one without, and a four-hearing group without, in this carry order"""
    with_alt, no_alt = alt_reply(17, ALT_FT[0], tc=9), alt_reply(17, ALT_FT[0], seed=1, tc=19)
    rx = dict(RX3)
    rx.update({s + 3: p for s, p in receivers(4, seed=TM.GOOD_SEED[4]).items()})
    c = Carry().hear(AIDED[0], rx, [0, 1, 2], 0.10, *with_alt).hear(AIDED[0], rx, [0, 1, 2], 0.15, *no_alt)
    c.hear(AIRCRAFT[0], rx, [3, 4, 5, 6], 0.20, IDENT, IDENT_LONG)
    return c, rx


def test_three_hearings_beside_four(sim):
    """Selection: with ADSB_MLAT_ALTITUDE and min_rx 3 the aided three and the four are rows, the unaided three is none; first[]
    and the counts follow; without the flag (min_rx 4) only the four; the count query and both -ENOSPC paths write nothing."""
    c, rx = three_and_four()
    both = dict(flags=RESTART | ALTITUDE, min_rx=3)
    fixes, aux, exp = check(sim, "3+4", c, rx, truth=[AIDED[0], AIRCRAFT[0]], **both)
    assert fixes["n_rx"].tolist() == [3, 4] and fixes["first"].tolist() == [0, 3] and aux["alt_ft"].tolist() == [ALT_FT[0], -1]
    assert aux["flags"][0] == RR.AUX_AIDED and not aux["flags"][1] & RR.AUX_AIDED
    assert [h for h, _ in MR.groups(c.replay_list(), WINDOW)] == [0, 3, 6]
    only4, _, _ = check(sim, "3+4", c, rx, truth=AIRCRAFT[0], flags=RESTART)
    assert only4["n_rx"].tolist() == [4] and only4["first"].tolist() == [0]
    assert check(sim, "3+4", c, rx, truth=AIRCRAFT[0], **dict(both, min_rx=4))[0]["n_rx"].tolist() == [4]
    for cap, member_cap in ((1, 7), (2, 6), (0, 0)):
        rc, fixes, aux, ms, mt, heads, nf, nm = run_rule(sim, c, rx, cap=cap, member_cap=member_cap, **both)
        assert rc == -28 and (nf, nm) == (2, 7)
        assert (fixes["first"] == -77).all() and (aux["tries"] == -77).all() and (ms == -77).all() and (mt == -77.0).all()
    rc, fixes, aux, ms, mt, heads, nf, nm = run_rule(sim, c, rx, cap=2, member_cap=7, want_aux=False, **both)
    assert rc == 0 and (nf, nm) == (2, 7) and (fixes["first"] >= 0).all() and (aux["tries"] == -77).all()      # aux may be NULL


FORMATS = [(0, {}), (4, {}), (16, {}), (20, {}), (17, dict(tc=9)), (17, dict(tc=18)), (17, dict(tc=8)), (17, dict(tc=19)), (4, dict(q=0)),
           (4, dict(m=1)), (20, dict(raw=0)), (17, dict(tc=11, q=0)), (17, dict(tc=11, raw=0)), (5, {}), (21, {}), (11, {}), (18, dict(tc=11))]


@pytest.mark.parametrize("which", range(len(FORMATS)))
def test_altitude_formats(sim, which):
    """Each format that announces an altitude, and the non-cases: type codes 8 and 19, Q = 0, M = 1, a zero field, DF 5 / 21 / 11
    / 18.  alt_ft is the replay's, the device function's, and the reference-pinned decoder rule's (tests/decode_replay.py: ac13
    over bits 19..31, ac12 over bits 40..51); three hearings are a row iff there is an altitude."""
    df, kw = FORMATS[which]
    fields = dict(kw)
    if df == 18:
        b, long_ = alt_reply(17, ALT_FT[1], **fields)
        b[0] = (18 << 3) | (b[0] & 7)
    elif df in (5, 21, 11):
        b, long_ = reply(df, 3)
    else:
        b, long_ = alt_reply(df, ALT_FT[1], **fields)
    bits = DR.AR._bits(b)
    if df in (0, 4, 16, 20):
        decoder = DR.ac13(DR.f(bits, 19, 13))
    elif df == 17 and 9 <= DR.f(bits, 32, 5) <= 18:
        decoder = DR.ac12(DR.f(bits, 40, 12))
    else:
        decoder = -1
    plain = not kw or set(kw) == {"tc"} and kw["tc"] in (9, 18)
    want = ALT_FT[1] if plain and df in (0, 4, 16, 20, 17) else -1
    assert decoder == want == RR.alt_ft_of(MR.payload_of(b, long_)) == sim.sim_mlat_alt_ft(b.ctypes.data_as(vp)), (df, kw, decoder)
    c = Carry().hear(AIDED[1], RX3, range(3), 0.25, b, long_)
    fixes, aux, exp = check(sim, "formats", c, RX3, flags=ALTITUDE, min_rx=3, converge=want != -1)
    assert aux["alt_ft"].tolist() == ([want] if want != -1 else [])
    c4 = Carry().hear(AIDED[1], receivers(4, seed=TM.GOOD_SEED[4]), range(4), 0.25, b, long_)
    fixes, aux, exp = check(sim, "formats4", c4, receivers(4, seed=TM.GOOD_SEED[4]), flags=RESTART | ALTITUDE, min_rx=3)
    assert aux["alt_ft"].tolist() == [want] and bool(aux["flags"][0] & RR.AUX_AIDED) == (want != -1)
    # without ADSB_MLAT_ALTITUDE no payload is read
    assert check(sim, "formats4", c4, receivers(4, seed=TM.GOOD_SEED[4]), flags=RESTART)[1]["alt_ft"].tolist() == [-1]


def test_all_receivers_at_one_point_is_singular(sim):
    """Every row of J is (1, 0, 0, -1): the second pivot is 0 whatever the damping; the restart's run from 30 km is singular too."""
    rx = {s: (MR.WGS_A, 0.0, 0.0) for s in range(4)}
    c = Carry()
    for s in range(4):
        c.add(T0 + 1e-4, IDENT, IDENT_LONG, s)
    fixes, aux, exp = check(sim, "singular", c, rx, converge=False)
    assert fixes["status"].tolist() == [N.MLAT_SINGULAR] and fixes["iters"][0] == 0 and aux["tries"][0] == 0
    assert aux["flags"][0] == RR.AUX_RESTARTED and (fixes["x"][0], fixes["y"][0], fixes["z"][0]) == (MR.WGS_A + 10000.0, 0.0, 0.0)
    fixes, aux, exp = check(sim, "singular", c, rx, converge=False, flags=0)
    assert fixes["status"].tolist() == [N.MLAT_SINGULAR] and aux["flags"][0] == 0


# (receivers, seed, aircraft): found on the CPU with the replay alone; the float64 and longdouble runs agree on every decision
RESTARTS = {"mirror": (4, 15, 0), "far": (4, 23, 2), "not kept": (4, 3, 1), "no end": (4, 11, 0)}


@pytest.mark.parametrize("kind", sorted(RESTARTS))
def test_the_restart(sim, kind):
    """mirror: the first run ends OK below the centroid plane, the run from the mirror point ends on the truth and is kept.
    far: the first run does not end, the run from 30 km does and is kept.  not kept: the first run ends below the plane and so
    does the second -- the first's result stands.  no end: neither run ends.  Without ADSB_MLAT_RESTART: the first run alone."""
    n, seed, k = RESTARTS[kind]
    rx = receivers(n, seed=seed)
    c = Carry().hear(AIRCRAFT[k], rx, range(n), 0.25, IDENT, IDENT_LONG)
    kept = kind in ("mirror", "far")
    fixes, aux, exp = check(sim, kind, c, rx, truth=AIRCRAFT[k] if kept else None, converge=kind != "no end")
    first, _, exp1 = check(sim, kind, c, rx, converge=kind not in ("far", "no end"), flags=0)
    e = exp[0]
    assert aux["flags"][0] == (RR.AUX_RESTARTED | (RR.AUX_SECOND_KEPT if kept else 0)) and exp1[0]["aux_flags"] == 0
    assert e["first_status"] == exp1[0]["status"] == first["status"][0] == (RR.OK if kind in ("mirror", "not kept") else RR.NO_CONVERGE)
    assert aux["tries"][0] > exp1[0]["tries"]
    if kept:
        assert aux["up_m"][0] > 0 and fixes["status"][0] == N.MLAT_OK and float(np.sqrt(((e["p"] - AIRCRAFT[k]) ** 2).sum())) < 1e-3
    else:
        assert fixes[["x", "y", "z", "status", "iters"]].tobytes() == first[["x", "y", "z", "status", "iters"]].tobytes()
    if kind in ("mirror", "not kept"):
        assert exp1[0]["up_m"] < 0


def test_the_argument_table(sim):
    """-EINVAL: an unknown solver, flag or reserved value; flags with _GN; min_rx below the bound; a weight that is not finite
    and positive where it is read; NaN bounds"""
    c, rx = three_and_four()
    ok = dict(solver=LM, flags=RESTART | ALTITUDE, min_rx=3, alt_weight=1.0)
    assert run_rule(sim, c, rx, **ok)[0] == 0
    for bad in (dict(solver=2), dict(solver=-1), dict(flags=4), dict(flags=RESTART | 8), dict(flags=-1), dict(reserved=1), dict(min_rx=2),
                dict(flags=RESTART, min_rx=3), dict(flags=0, min_rx=3), dict(alt_weight=0.0), dict(alt_weight=-1.0), dict(alt_weight=np.inf),
                dict(alt_weight=np.nan), dict(solver=GN, flags=RESTART, min_rx=4), dict(solver=GN, flags=ALTITUDE, min_rx=4),
                dict(solver=GN, flags=0, min_rx=3), dict(t_lo=np.nan), dict(t_hi=np.nan)):
        rc, fixes, aux, *_ = run_rule(sim, c, rx, **dict(ok, **bad))
        assert rc == -22 and (fixes["first"] == -77).all() and (aux["tries"] == -77).all(), bad
    assert run_rule(sim, c, rx, solver=LM, flags=RESTART, min_rx=4, alt_weight=np.nan)[0] == 0      # not read without the flag
    assert run_rule(sim, c, rx, solver=GN, flags=0, min_rx=4, alt_weight=np.nan)[0] == 0


# ---- convergence, anchored to the undamped rule ------------------------------------------------------------------------------
LAT1, LON1, GEOMETRIES = 50.0, 8.0, 48


def world(n, seed):
    """48 geometries: n receivers uniform in +-0.9 deg x +-1.4 deg around 50 N 8 E, 0 .. 2500 m up, and an aircraft in the same
    box at 1000 .. 12000 m -> [(receivers [n, 3], aircraft, its height in m)]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(GEOMETRIES):
        rx = np.array([MR.geodetic_to_ecef(LAT1 + rng.uniform(-0.9, 0.9), LON1 + rng.uniform(-1.4, 1.4), rng.uniform(0.0, 2500.0)) for _ in range(n)])
        alt = (LAT1 + rng.uniform(-0.9, 0.9), LON1 + rng.uniform(-1.4, 1.4), rng.uniform(1000.0, 12000.0))
        out.append((rx, MR.geodetic_to_ecef(*alt), alt[2]))
    return out


def world_carry(n, seed):
    """The 48 geometries in one carry: geometry g is heard by streams g n .. g n + n - 1, 5 ms after the one before, with exact
    arrival times -> (Carry, rx, truths)"""
    c, rx, truths = Carry(), {}, []
    for g, (R, p, _) in enumerate(world(n, seed)):
        for s in range(n):
            rx[g * n + s] = tuple(R[s])
        c.hear(p, rx, range(g * n, g * n + n), 0.005 * g, IDENT, IDENT_LONG)
        truths.append(p)
    return c, rx, truths


def hit(e, truth):
    return e["status"] == RR.OK and float(np.sqrt(((np.asarray(e["p"], np.float64) - truth) ** 2).sum())) < 1.0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n", [6, 8])
def test_the_damped_rule_converges_where_the_undamped_one_does(sim, n, seed):
    """48 random geometries of n receivers: every geometry that tests/mlat_replay.py's undamped solve puts within 1 m of the
    truth is within 1 m under the damped rule with restart, and the damped rule hits more; both counted by the replays.  The
    emulation's statuses are the replay's, and where the replay hits, so does the emulation."""
    c, rx, truths = world_carry(n, seed)
    lst = c.replay_list()
    old = MR.mlat(lst, WINDOW, rx)[0]
    new = RR.mlat(lst, WINDOW, rx)[0]
    assert len(old) == len(new) == GEOMETRIES and [e["head"] for e in old] == [e["head"] for e in new]
    old_hits, new_hits = [hit(e, t) for e, t in zip(old, truths)], [hit(e, t) for e, t in zip(new, truths)]
    print("%d receivers, seed %d: undamped %d, damped with restart %d of %d" % (n, seed, sum(old_hits), sum(new_hits), GEOMETRIES))
    assert all(b for a, b in zip(old_hits, new_hits) if a) and sum(new_hits) > sum(old_hits)
    rc, fixes, aux, ms, mt, heads, nf, nm = run_rule(sim, c, rx)
    assert rc == 0 and nf == GEOMETRIES and fixes["status"][:nf].tolist() == [e["status"] for e in new]
    for f, e, t, h in zip(fixes[:nf], new, truths, new_hits):
        if h:
            assert float(np.sqrt(((np.array([f["x"], f["y"], f["z"]]) - t) ** 2).sum())) < 1.0 + TOL


# ---- the periodic carry ----------------------------------------------------------------------------------------------------------
# tests/test_mlat.py's scheme with a denser period, so that few entries make many groups: PERIOD = 15 entries (coprime to 64 and
# 256) within 1 ms, repeated every SPACING = 2^-7 s from EPOCH = 1024 s on; every shift is exact, so period k's solver inputs are
# bit for bit period 0's.
EPOCH, SPACING, PERIOD = TM.EPOCH, TM.SPACING, 15
PER_HEADS, PER_FIXES, PER_MEMBERS = 5, 3, 11
RULE_P = dict(flags=RESTART | ALTITUDE, min_rx=3)


def period0():
    """-> Carry: a four-hearing group without an altitude (restart), a four-hearing short reply with one (aided), a
    three-hearing group with an altitude (aided), a three-hearing group without (no row), a filler"""
    rx = RX8
    at = lambda p, s: EPOCH + float(np.sqrt(((np.asarray(p) - np.asarray(rx[s])) ** 2).sum())) / MR.C      # noqa: E731
    c = Carry()
    for s in (0, 1, 2, 3):
        c.add(at(AIRCRAFT[0], s), IDENT, IDENT_LONG, s)
    short = alt_reply(4, ALT_FT[1], seed=2)
    for s in (4, 5, 6, 7):
        c.add(at(AIDED[1], s), short[0], False, s)
    three = alt_reply(17, ALT_FT[0], seed=3, tc=12)
    for s in (1, 3, 5):
        c.add(at(AIDED[0], s) + 1e-6, three[0], True, s)
    bare = alt_reply(17, ALT_FT[0], seed=4, tc=19)
    for s in (0, 2, 6):
        c.add(at(AIDED[0], s) + 2e-6, bare[0], True, s)
    c.add(EPOCH + 1e-5, TM.fillers(1, 15)[0], True, 7)
    ts = c.arrays()[0]
    assert len(ts) == PERIOD and (np.diff(ts) > 0).all() and EPOCH < ts[0] and ts[-1] - ts[0] < 1e-3
    return c


def periodic(n_periods):
    p0 = period0().arrays()
    shift = np.arange(n_periods) * SPACING
    ts = (p0[0][None, :] + shift[:, None]).ravel()
    assert ts[-1] < 2 * EPOCH and (ts.reshape(n_periods, PERIOD) - shift[:, None] == p0[0]).all()
    return (ts, np.tile(p0[1], (n_periods, 1)).copy(), np.tile(p0[2], n_periods).copy(), np.tile(p0[3], n_periods).copy())


def check_periodic(sim, case, n_periods):
    """Period 0 alone against the replay; one call over n_periods periods: its period 0 is that call's rows byte for byte, and
    every period k is period 0 -- `first` + 11 k, ts and member_ts + k SPACING exactly, every other field of the fix and of the
    aux row bit for bit, t_tx within one spacing of the shifted value."""
    alone, alone_aux, exp = check(sim, case, period0(), RX8, converge=False, **RULE_P)
    assert len(exp) == PER_FIXES and sum(e["n_rx"] for e in exp) == PER_MEMBERS and alone_aux["alt_ft"].tolist() == [-1, ALT_FT[0], ALT_FT[1]]
    rc, fixes, aux, ms, mt, heads, nf, nm = run_rule_arrays(sim, *periodic(n_periods), RX8, **RULE_P)
    assert rc == 0 and (nf, nm, len(heads)) == (n_periods * PER_FIXES, n_periods * PER_MEMBERS, n_periods * PER_HEADS), case
    ks = np.arange(n_periods)
    F, A = fixes[:nf].reshape(n_periods, PER_FIXES), aux[:nf].reshape(n_periods, PER_FIXES)
    assert F[0].tobytes() == alone.tobytes() and A[0].tobytes() == alone_aux.tobytes(), case
    assert np.array_equal(heads.reshape(n_periods, PER_HEADS), heads[:PER_HEADS][None, :] + PERIOD * ks[:, None]), case
    for name in ("bits", "flags", "icao", "n_rx", "n_heard", "status", "iters"):
        assert (F[name] == F[0][name][None]).all(), (case, name)
    assert (A.view(np.uint8).reshape(n_periods, -1) == A[0].view(np.uint8).reshape(1, -1)).all(), case
    assert np.array_equal(F["first"], F[0]["first"][None, :] + PER_MEMBERS * ks[:, None]), case
    assert np.array_equal(F["ts"], F[0]["ts"][None, :] + SPACING * ks[:, None]), case
    M_s, M_t = ms[:nm].reshape(n_periods, PER_MEMBERS), mt[:nm].reshape(n_periods, PER_MEMBERS)
    assert (M_s == M_s[0][None, :]).all() and np.array_equal(M_t, M_t[0][None, :] + SPACING * ks[:, None]), case
    for name in ("x", "y", "z", "rms_m"):
        assert np.array_equal(F[name].view(np.uint64), np.broadcast_to(F[0][name].view(np.uint64)[None, :], F[name].shape)), (case, name)
    shifted = F[0]["t_tx"][None, :] + SPACING * ks[:, None]
    assert (np.abs(F["t_tx"] - shifted) <= np.spacing(shifted)).all(), case
    return fixes[:nf], aux[:nf], heads


def test_a_periodic_carry(sim):
    """Twenty periods, 300 entries: more than one workgroup of heads and of groups, and a second grid-stride round with the
    emulator driver's two workgroups."""
    check_periodic(sim, "periodic", 20)


def test_the_replays_own_sensitivity():
    """Runs after the cases above: the largest float64-vs-longdouble distance of the replay over them is what the module's
    docstring states, and TOL follows from it."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("this platform's long double is a double: the sensitivity was measured where it is wider")
    assert measured, "the cases above ran"
    worst = max(measured, key=lambda m: m[1])
    print("replay float64 vs longdouble: worst %.3g m in case %r over %d fixes; TOL %.3g m" % (worst[1], worst[0], len(measured), TOL))
    assert worst[1] <= SENS and TOL == 2e-3


# ---- build facts -----------------------------------------------------------------------------------------------------------
def test_kernel_resources_mlat_rule():
    """The fifth translation unit's report: exactly the two new kernels, neither with scratch, spills or LDS; its figures are
    DESIGN.md §3i's.  (adsb_mlat.hip's report, which tests/test_mlat.py holds to its seven kernels, is untouched.)"""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES_MLAT_RULE))
    name = lambda k: re.search(r"k_mlat_[a-z_]+?(?=E)", k).group(0)      # noqa: E731
    assert sorted(name(k) for k in res) == ["k_mlat_groups_rule", "k_mlat_solve_lm"], sorted(res)
    design = open(os.path.join(HERE, "..", "DESIGN.md")).read()
    for k, v in res.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["lds_bytes_per_block"] == 0, (k, v)
        assert "%s: %d VGPRs" % (name(k), v["vgprs"]) in design, (name(k), v["vgprs"])
    assert B.MLAT_RULE_SOURCE == "adsb_mlat_rule.hip" and all(d in B.DEPS for d in ("adsb_mlat_rule.hip", "adsb_mlat_rule.h", "adsb_mlat_rule_device.h"))
    assert not any("k_mlat" in k and ("_rule" in k or "_lm" in k) for k in json.load(open(B.RES_MLAT)))


def test_the_sizing_rule(sim):
    """adsb_mlat_rule.h's layout_rule(): layout()'s parts with nc / 3 + 1 fixes, and as many aux rows behind member_ts"""
    for nc, ns in ((1, 1), (2, 1), (3, 3), (255, 3), (256, 8), (257, 8), (100000, 64)):
        chunks = (nc + 255) // 256 + 1
        parts = [16, 16, 16, nc * 4, chunks * 4, chunks * 4, nc * 4, nc * 4, nc * 4, nc * 4, ns * 24, (nc // 3 + 1) * 88, nc * 4, nc * 8,
                 (nc // 3 + 1) * 32]
        assert sim.sim_mlat_rule_layout_bytes(nc, ns) == sum((p + 255) // 256 * 256 for p in parts)
        assert sim.sim_mlat_rule_layout_bytes(nc, ns) > sim.sim_mlat_layout_bytes(nc, ns)


def test_constants_and_export_names():
    hdr = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_ABI_VERSION (\d+)", hdr).group(1) == "5" and N.ABI_VERSION == 5
    for name, value in (("SOLVER_GN", 0), ("SOLVER_LM", 1), ("RESTART", 1), ("ALTITUDE", 2), ("AUX_AIDED", 1), ("AUX_RESTARTED", 2),
                        ("AUX_SECOND_KEPT", 4)):
        assert int(re.search(r"#define ADSB_MLAT_%s (\d+)u?$" % name, hdr, re.M).group(1)) == getattr(N, "MLAT_" + name) == value
    assert (RR.SOLVER_GN, RR.SOLVER_LM, RR.RESTART, RR.ALTITUDE) == (N.MLAT_SOLVER_GN, N.MLAT_SOLVER_LM, N.MLAT_RESTART, N.MLAT_ALTITUDE)
    assert (RR.AUX_AIDED, RR.AUX_RESTARTED, RR.AUX_SECOND_KEPT) == (N.MLAT_AUX_AIDED, N.MLAT_AUX_RESTARTED, N.MLAT_AUX_SECOND_KEPT)
    assert "adsb_stream_mlat_rule" in N.EXPORTS and re.search(r"^int adsb_stream_mlat_rule\(adsb_ctx\* ctx", hdr, re.M)
    assert callable(N.Context.stream_mlat_rule) and ctypes.sizeof(N.MLAT_RULE) == 24
    assert [f for f, _ in N.MLAT_RULE._fields_] == ["solver", "flags", "min_rx", "reserved", "alt_weight"]
    assert list(N.MLAT_AUX_DTYPE.names) == ["up_m", "lambda", "alt_ft", "tries", "flags", "reserved"]
    for struct, names in (("adsb_mlat_rule", [f for f, _ in N.MLAT_RULE._fields_]), ("adsb_mlat_aux", list(N.MLAT_AUX_DTYPE.names))):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        assert re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S)) == names, struct
    for phrase in ("THE DAMPED RULE", "THE UNTESTED LAST STEP", "THE RESTART", "THE ALTITUDE ROW"):
        assert phrase in hdr
    assert "altitude-aided three-receiver fixes are not provided" not in hdr
