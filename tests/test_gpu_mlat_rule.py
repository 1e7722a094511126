"""adsb_stream_mlat_rule on the MI355X, through the C ABI, on tests/test_gpu_mlat.py's six-receiver carry: the damped and the
aided call equal tests/mlat_rule_replay.py -- the header's DAMPED RULE in plain Python -- fed the DELIVERED records, with
test_mlat_rule.py's compare() and tolerance; ADSB_MLAT_SOLVER_GN is adsb_stream_mlat byte for byte; the call changes nothing
a caller can see; the argument table, the count query and -ENOSPC; Context.stream_mlat_rule and Receivers.mlat(solver="damped").
The CPU half (emulated kernels, every case) is tests/test_mlat_rule.py."""
import ctypes

import numpy as np
import pytest

import mlat_rule_replay as RR
import test_gpu_mlat as G
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from test_gpu_mlat import CUTS_THREE, CUTS_WHOLE, N_REPLIES, N_RX, RX, STARTS, WINDOW, P, native      # noqa: F401
from test_mlat_rule import TOL, compare

pytestmark = pytest.mark.gpu

ENOSPC, EINVAL = 28, 22
LM, GN, RESTART, ALTITUDE = N.MLAT_SOLVER_LM, N.MLAT_SOLVER_GN, N.MLAT_RESTART, N.MLAT_ALTITUDE


def rule(solver=LM, flags=RESTART, min_rx=4, reserved=0, alt_weight=1.0):
    return N.MLAT_RULE(solver, flags, min_rx, reserved, alt_weight)


def replay(delivered, starts, rx, **kw):
    lst = G.carry_of(delivered, starts)
    exp, ems, emt = RR.mlat(lst, WINDOW, rx, **kw)
    return exp, ems, emt, RR.mlat(lst, WINDOW, rx, ft=np.longdouble, **kw)[0]


def test_the_damped_and_the_aided_call(native):
    """Every reply is a six-hearing group at the aircraft: the damped call with restart ends on it; the aided call takes the
    altitude the extended squitters' random message fields happen to announce (about half have Q = 1) at a weight of 0.01 and
    equals the replay row for row; both leave the state's digest as it was, and a second call is byte-identical."""
    ctx = G.mlat_ctx()
    delivered = G.push(ctx, G.sources(), CUTS_THREE)
    before = G.digest(ctx)
    fixes, aux, ms, mt = ctx.stream_mlat_rule(rule())
    assert G.digest(ctx) == before
    again = ctx.stream_mlat_rule(rule(), cap=len(fixes), member_cap=len(ms))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (fixes, aux, ms, mt)))
    exp, ems, emt, ld = replay(delivered, STARTS, RX, flags=RESTART)
    compare("damped", fixes, aux, ms, mt, exp, ems, emt, truth=P, exp_ld=ld, converge=True)
    assert len(fixes) >= N_REPLIES - 2 and (fixes["status"] == N.MLAT_OK).all() and (aux["alt_ft"] == -1).all() and (aux["up_m"] > 0).all()
    p = np.stack([fixes["x"], fixes["y"], fixes["z"]], axis=1)
    assert float(np.sqrt(((p - P) ** 2).sum(axis=1)).max()) <= TOL + max(float(np.sqrt(((e["p"] - P) ** 2).sum())) for e in exp)

    aided = rule(flags=RESTART | ALTITUDE, min_rx=3, alt_weight=0.01)
    fixes_a, aux_a, ms_a, mt_a = ctx.stream_mlat_rule(aided)
    exp, ems, emt, ld = replay(delivered, STARTS, RX, flags=RESTART | ALTITUDE, min_rx=3, alt_weight=0.01)
    compare("aided", fixes_a, aux_a, ms_a, mt_a, exp, ems, emt, exp_ld=ld, converge=False)
    with_alt = (aux_a["flags"] & N.MLAT_AUX_AIDED) != 0
    assert 20 < with_alt.sum() < len(fixes_a) - 20 and np.array_equal(with_alt, aux_a["alt_ft"] != -1)
    assert fixes_a[~with_alt].tobytes() == fixes[~with_alt].tobytes()      # an unaided group's row does not depend on the flag
    assert G.digest(ctx) == before
    ctx.close()


def test_three_positioned_receivers(native):
    """Only receivers 0 .. 2 have a position: every group uses three hearings of six heard, and is a row iff its reply announces
    an altitude -- selection, first[] and the counts through the host's compaction and its nc / 3 sizing."""
    ctx = G.mlat_ctx(corr="None", positions=range(3))
    delivered = G.push(ctx, [G.sources()[0]] * N_RX, CUTS_WHOLE)
    rx3 = {s: RX[s] for s in range(3)}
    aided = rule(flags=ALTITUDE, min_rx=3, alt_weight=0.5)
    fixes, aux, ms, mt = ctx.stream_mlat_rule(aided)
    exp, ems, emt, ld = replay(delivered, STARTS, rx3, flags=ALTITUDE, min_rx=3, alt_weight=0.5)
    compare("three", fixes, aux, ms, mt, exp, ems, emt, exp_ld=ld, converge=False)
    assert 20 < len(fixes) < N_REPLIES - 20 and (fixes["n_rx"] == 3).all() and (fixes["n_heard"] == N_RX).all() and (aux["alt_ft"] != -1).all()
    assert np.array_equal(fixes["first"], 3 * np.arange(len(fixes))) and len(ms) == 3 * len(fixes)
    assert len(ctx.stream_mlat_rule(rule(flags=ALTITUDE, min_rx=4))[0]) == 0 and len(ctx.stream_mlat()[0]) == 0
    ctx.close()


def raw_rule(ctx, r, cap, member_cap, t_lo=-np.inf, t_hi=np.inf, aux=True):
    """adsb_stream_mlat_rule with buffers of exactly cap / member_cap entries and a guard entry behind each"""
    fixes, rows = np.zeros(cap + 1, dtype=N.MLAT_DTYPE), np.zeros(cap + 1, dtype=N.MLAT_AUX_DTYPE)
    fixes.view(np.uint8)[:] = 0xA5
    rows.view(np.uint8)[:] = 0xA5
    ms, mt = np.full(member_cap + 1, -77, np.int32), np.full(member_cap + 1, -77.0)
    n, m = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = ctx.lib.adsb_stream_mlat_rule(ctx._h, t_lo, t_hi, ctypes.byref(r) if r is not None else None, fixes.ctypes.data,
                                       rows.ctypes.data if aux else None, cap, ctypes.byref(n), ms.ctypes.data, mt.ctypes.data, member_cap,
                                       ctypes.byref(m))
    return rc, n.value, m.value, fixes, rows, ms, mt


def test_gauss_newton_the_argument_table_and_no_space(native):
    ctx = G.mlat_ctx(corr="None")
    assert ctx.stream_mlat_rule(rule())[0].shape == (0,) and raw_rule(ctx, rule(), 0, 0)[:3] == (0, 0, 0)      # an empty carry
    G.push(ctx, [G.sources()[0]] * N_RX, CUTS_WHOLE)
    before = G.digest(ctx)
    # _GN with no flags is adsb_stream_mlat, byte for byte, whatever min_rx and the range
    plain = ctx.stream_mlat()
    mid = float(plain[0]["ts"][len(plain[0]) // 2])
    for kw in (dict(), dict(min_rx=N_RX), dict(min_rx=N_RX + 1), dict(t_lo=mid), dict(t_hi=mid)):
        want = ctx.stream_mlat(**kw)
        got = ctx.stream_mlat_rule(rule(GN, 0, kw.get("min_rx", 4), 0, float("nan")), **{k: v for k, v in kw.items() if k != "min_rx"})
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, (got[0], got[2], got[3]))), kw
        assert (got[1]["alt_ft"] == -1).all() and not got[1]["tries"].any() and not got[1]["flags"].any()
    n, m = len(plain[0]), len(plain[1])
    for cap, member_cap in ((0, 0), (n - 1, m), (n, m - 1)):
        assert raw_rule(ctx, rule(GN, 0), cap, member_cap)[:3] == G.raw_mlat(ctx, cap, member_cap)[:3] == (-ENOSPC, n, m)
    # the argument table
    for bad in (None, rule(solver=2), rule(solver=-1), rule(flags=4), rule(flags=-1), rule(reserved=7), rule(min_rx=3), rule(flags=ALTITUDE, min_rx=2),
                rule(flags=ALTITUDE, alt_weight=0.0), rule(flags=ALTITUDE, alt_weight=float("inf")), rule(flags=ALTITUDE, alt_weight=float("nan")),
                rule(GN, RESTART), rule(GN, ALTITUDE), rule(GN, 0, 3)):
        rc, _, _, fixes, rows, ms, mt = raw_rule(ctx, bad, n, m)
        assert rc == -EINVAL and (fixes.view(np.uint8) == 0xA5).all() and (rows.view(np.uint8) == 0xA5).all() and (ms == -77).all(), bad
    assert raw_rule(ctx, rule(), n, m, t_lo=float("nan"))[0] == -EINVAL and raw_rule(ctx, rule(), n, m, t_hi=float("nan"))[0] == -EINVAL
    c2 = N.Context(G.FS, G.THR, flags=G.SD | G.SH)
    c2.open_streams(2)
    assert G._code(c2.stream_mlat_rule, rule()) == -EINVAL                # a context without the flag
    c2.close()
    # the count query and both -ENOSPC paths of the damped call: the counts, and nothing written
    for cap, member_cap in ((0, 0), (n - 1, m), (n, m - 1)):
        rc, n2, m2, fixes, rows, ms, mt = raw_rule(ctx, rule(), cap, member_cap)
        assert rc == -ENOSPC and (n2, m2) == (n, m)
        assert (fixes.view(np.uint8) == 0xA5).all() and (rows.view(np.uint8) == 0xA5).all() and (ms == -77).all() and (mt == -77.0).all()
    rc, n2, m2, fixes, rows, ms, mt = raw_rule(ctx, rule(), n, m)
    assert rc == 0 and (n2, m2) == (n, m) and (fixes[n:].view(np.uint8) == 0xA5).all() and (rows[n:].view(np.uint8) == 0xA5).all()
    assert ms[m] == -77 and mt[m] == -77.0 and (fixes["status"][:n] == N.MLAT_OK).all()
    rc, n2, m2, fixes2, rows2, ms2, mt2 = raw_rule(ctx, rule(), n, m, aux=False)      # aux may be NULL
    assert rc == 0 and fixes2.tobytes() == fixes.tobytes() and ms2.tobytes() == ms.tobytes() and (rows2.view(np.uint8) == 0xA5).all()
    full = ctx.stream_mlat_rule(rule(), cap=1, member_cap=1)           # the Python call asks again with what is needed
    assert full[0].tobytes() == fixes[:n].tobytes() and full[1].tobytes() == rows[:n].tobytes() and full[2].tobytes() == ms[:m].tobytes()
    assert G.digest(ctx) == before
    ctx.close()


def test_every_refusal_names_the_entry_point_that_was_called(native):
    """Each -EINVAL of adsb_stream_mlat and adsb_stream_mlat_rule, on four open streams and an empty carry (host work only): the
    return code, and the context's error text -- the texts are those of the source before the two calls shared one body, each
    with the name of the entry point that was called in front."""
    ctx = N.Context(G.FS, G.THR, flags=G.SD | G.SH | G.DD)
    ctx.open_streams(4)
    nan, inf = float("nan"), float("inf")
    n, m = ctypes.c_int32(-1), ctypes.c_int32(-1)

    def plain(t_lo=-inf, t_hi=inf, min_rx=4, n_fixes=ctypes.byref(n)):
        return ctx.lib.adsb_stream_mlat(ctx._h, t_lo, t_hi, min_rx, None, 0, n_fixes, None, None, 0, ctypes.byref(m))

    def ruled(r, t_lo=-inf, t_hi=inf, n_fixes=ctypes.byref(n)):
        return ctx.lib.adsb_stream_mlat_rule(ctx._h, t_lo, t_hi, ctypes.byref(r) if r is not None else None, None, None, 0, n_fixes, None, None, 0,
                                             ctypes.byref(m))

    missing = "n_fixes / n_members, or the arrays for cap / member_cap > 0, missing"
    cases = [("adsb_stream_mlat", lambda: plain(t_lo=nan), "a bound is NaN"),
             ("adsb_stream_mlat", lambda: plain(t_hi=nan), "a bound is NaN"),
             ("adsb_stream_mlat", lambda: plain(min_rx=3), "min_rx < 4 (three-receiver fixes are not provided)"),
             ("adsb_stream_mlat", lambda: plain(n_fixes=None), missing),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(), t_lo=nan), "a bound is NaN"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(), t_hi=nan), "a bound is NaN"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(), n_fixes=None), missing),
             ("adsb_stream_mlat_rule", lambda: ruled(None), "rule is NULL"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(min_rx=3)), "min_rx < 4 (< 3 with ADSB_MLAT_ALTITUDE)"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(flags=ALTITUDE, min_rx=2)), "min_rx < 4 (< 3 with ADSB_MLAT_ALTITUDE)"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(GN, 0, 3)), "min_rx < 4 (< 3 with ADSB_MLAT_ALTITUDE)"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(solver=2)), "unknown solver"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(flags=4)), "unknown flags"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(GN, RESTART)), "flags need ADSB_MLAT_SOLVER_LM"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(reserved=7)), "reserved is not 0"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(flags=ALTITUDE, alt_weight=0.0)), "alt_weight is not finite and > 0"),
             ("adsb_stream_mlat_rule", lambda: ruled(rule(flags=ALTITUDE, alt_weight=nan)), "alt_weight is not finite and > 0")]
    for api, call, what in cases:
        assert call() == -EINVAL, (api, what)
        text = ctx.lib.adsb_last_error(ctx._h).decode()
        assert text.startswith(api + ": ") and text == api + ": " + what, (api, what, text)
    assert plain() == 0 and ruled(rule()) == 0 and ruled(rule(GN, 0)) == 0 and (n.value, m.value) == (0, 0)      # the empty carry
    ctx.close()
    c2 = N.Context(G.FS, G.THR, flags=G.SD | G.SH | G.DD)                  # the two preambles' texts
    for api, call in (("adsb_stream_mlat", lambda: c2.lib.adsb_stream_mlat(c2._h, -inf, inf, 4, None, 0, ctypes.byref(n), None, None, 0, ctypes.byref(m))),
                      ("adsb_stream_mlat_rule", lambda: c2.lib.adsb_stream_mlat_rule(c2._h, -inf, inf, ctypes.byref(rule()), None, None, 0, ctypes.byref(n),
                                                                                      None, None, 0, ctypes.byref(m)))):
        assert call() == -EINVAL and c2.lib.adsb_last_error(c2._h).decode() == api + ": no streams (adsb_streams_open first)"
    c2.close()
    c3 = N.Context(G.FS, G.THR, flags=G.SD | G.SH)
    c3.open_streams(2)
    assert c3.lib.adsb_stream_mlat(c3._h, -inf, inf, 4, None, 0, ctypes.byref(n), None, None, 0, ctypes.byref(m)) == -EINVAL
    assert c3.lib.adsb_last_error(c3._h).decode() == "context created without ADSB_FLAG_STREAM_DEDUP"
    c3.close()


def test_the_front_end(native):
    """Receivers.mlat(solver="damped"): the fixes with alt_ft, up_m, tries and aux_flags added; the defaults are today's rows."""
    fe = frontend.FrontEnd(G.FS, G.THR, flags=G.SD | G.SH | G.DD)
    rx = fe.receivers(N_RX, fmt=N.FMT_FC32, starts=STARTS, shared=True, dedup=True, positions=G.LLA)
    rx.push([G.sources()[0]] * N_RX)
    rx.finish()
    plain, pms, pmt = rx.mlat()
    today = fe.ctx.stream_mlat()[0]
    assert "tries" not in plain.dtype.names and all(plain[name].tobytes() == today[name].tobytes() for name in N.MLAT_DTYPE.names)
    fixes, ms, mt = rx.mlat(solver="damped")
    raw, aux, rms, rmt = fe.ctx.stream_mlat_rule(rule())
    assert len(fixes) >= N_REPLIES - 2 and (fixes["status"] == N.MLAT_OK).all() and np.array_equal(ms, rms) and np.array_equal(mt, rmt)
    for name in N.MLAT_DTYPE.names:
        assert fixes[name].tobytes() == raw[name].tobytes(), name
    assert np.array_equal(fixes["tries"], aux["tries"]) and np.array_equal(fixes["up_m"], aux["up_m"]) and (fixes["alt_ft"] == -1).all()
    assert np.array_equal(fixes["aux_flags"], aux["flags"])
    assert np.abs(fixes["latitude"] - G.AIRCRAFT_LLA[0]).max() < 1e-6 and np.abs(fixes["altitude_m"] - G.AIRCRAFT_LLA[2]).max() < 0.1
    aided, _, _ = rx.mlat(solver="damped", altitude=True, alt_weight=0.01, min_rx=3, restart=False)
    want = fe.ctx.stream_mlat_rule(rule(flags=ALTITUDE, min_rx=3, alt_weight=0.01))
    assert np.array_equal(aided["alt_ft"], want[1]["alt_ft"]) and (aided["alt_ft"] != -1).any() and aided["x"].tobytes() == want[0]["x"].tobytes()
    with pytest.raises(ValueError):
        rx.mlat(solver="newton")
    rx.close()
    fe.ctx.close()
