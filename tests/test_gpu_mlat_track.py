"""The MLAT track store on the MI355X, through the C ABI: tests/test_gpu_mlat.py's six receivers (its fixture and helpers,
imported) hear twelve aircraft's replies, adsb_stream_mlat_track fuses the fixes per address on the device, and the store read
back equals tests/mlat_track_replay.py -- the header's MLAT TRACKS rule in plain Python -- fed the fixes and aux rows that
adsb_stream_mlat_rule delivered for the same rule and range: byte for byte, no tolerance.  The aircraft of that fixture stand
still, so v stays near 0; movement, every seam of the kernels and the merge are tests/test_mlat_track.py's (emulator) and
tests/test_gpu_mlat_track_device.py's (device).  The call changes nothing a caller can see but the store."""
import ctypes

import numpy as np
import pytest

import mlat_track_replay as R
import test_gpu_mlat as G
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from test_gpu_mlat import native      # noqa: F401

pytestmark = pytest.mark.gpu

ENOSPC, EINVAL = 28, 22
ROW = N.MLAT_TRACK_DTYPE
LM, GN, RESTART = N.MLAT_SOLVER_LM, N.MLAT_SOLVER_GN, N.MLAT_RESTART
inf = float("inf")


def rule(solver=LM, flags=RESTART, min_rx=4, reserved=0, alt_weight=1.0):
    return N.MLAT_RULE(solver, flags, min_rx, reserved, alt_weight)


@pytest.fixture(scope="module")
def pushed(native):      # noqa: F811
    """one context with the whole source pushed in three cuts; every test leaves its track store empty"""
    ctx = G.mlat_ctx()
    G.push(ctx, G.sources(), G.CUTS_THREE)
    yield ctx
    ctx.close()


def store(ctx):
    return ctx.stream_mlat_tracks(min_fixes=-(1 << 31))


@pytest.mark.parametrize("solver", ["damped", "gauss-newton"])
def test_the_tracks_equal_the_replay(pushed, solver):
    """stream_mlat_rule and stream_mlat_track with the same rule and range: the tracks are the replay's over the delivered fixes,
    the stats too, and the state's digest is unchanged; a second identical call changes no track and all its usable fixes are
    stale.  Under ADSB_MLAT_SOLVER_GN no aux row exists on the device and up_m is 0."""
    ctx = pushed
    r = rule() if solver == "damped" else rule(GN, 0)
    before = G.digest(ctx)
    fixes, aux, _, _ = ctx.stream_mlat_rule(r)
    assert len(fixes) >= G.N_REPLIES - 2 and (aux["up_m"] == 0.0).all() == (solver != "damped")
    stats = ctx.stream_mlat_track(r, N.mlat_track_rule())
    assert G.digest(ctx) == before
    tracks = {}
    exp_stats = R.update(tracks, fixes, aux, {})
    got = store(ctx)
    assert stats == exp_stats and got.tobytes() == R.rows(tracks, ROW).tobytes()
    assert stats["tracks"] == len(got) >= 12 and stats["taken"] > 100 and stats["rejected"] == 0
    es = got[(got["icao"] >= 0x4B1A00) & (got["icao"] < 0x4B1A00 + 12)]
    assert len(es) == 12 and (es["n_fixes"] >= 9).all()
    assert np.abs(np.stack([es[k] for k in "xyz"], 1) - G.P).max() < 1.0 and np.abs(np.stack([es["v" + k] for k in "xyz"], 1)).max() < 50.0
    again = ctx.stream_mlat_track(r, N.mlat_track_rule())
    assert store(ctx).tobytes() == got.tobytes() and G.digest(ctx) == before
    assert again["stale"] == again["eligible"] - again["unusable"] and again["taken"] == again["started"] == again["rejected"] == 0
    assert (again["fixes"], again["eligible"], again["unusable"], again["tracks"]) == (stats["fixes"], stats["eligible"], stats["unusable"], stats["tracks"])
    # the readout's filters and the Python call's second ask
    for min_fixes, cutoff in ((1, -inf), (3, -inf), (1, float(np.median(got["last_ts"]))), (50, -inf)):
        want = R.rows(tracks, ROW, min_fixes, cutoff)
        assert ctx.stream_mlat_tracks(min_fixes, cutoff).tobytes() == want.tobytes()
        assert ctx.stream_mlat_tracks(min_fixes, cutoff, cap=1).tobytes() == want.tobytes()
    ctx.reset_mlat_tracks()
    assert len(store(ctx)) == 0


def test_adjoining_ranges_give_the_store_of_one_call(pushed):
    """one call per cut of the push, over the adjoining ranges the cuts' times bound, against one call over everything"""
    ctx = pushed
    ctx.stream_mlat_track(rule(), N.mlat_track_rule())
    whole = store(ctx)
    ctx.reset_mlat_tracks()
    edges = [-inf] + [G.T0 + c / G.FS for c in G.CUTS_THREE[0]] + [inf]
    total = dict.fromkeys(R.STATS, 0)
    for lo, hi in zip(edges[:-1], edges[1:]):
        s = ctx.stream_mlat_track(rule(), N.mlat_track_rule(), lo, hi)
        assert s["fixes"] > 0
        for k in ("fixes", "eligible", "taken", "started", "stale"):
            total[k] += s[k]
    assert store(ctx).tobytes() == whole.tobytes() and total["stale"] == 0 and total["fixes"] >= G.N_REPLIES - 2
    # overlapping ranges: harmless
    ctx.stream_mlat_track(rule(), N.mlat_track_rule(), edges[1], inf)
    assert store(ctx).tobytes() == whole.tobytes()
    ctx.reset_mlat_tracks()


def test_expire_reset_and_close(native):      # noqa: F811
    ctx = G.mlat_ctx()
    G.push(ctx, G.sources(), G.CUTS_WHOLE)
    r = rule()
    fixes, aux, _, _ = ctx.stream_mlat_rule(r)
    ctx.stream_mlat_track(r, N.mlat_track_rule())
    tracks = {}
    R.update(tracks, fixes, aux, {})
    got = store(ctx)
    cut = float(np.sort(got["last_ts"])[len(got) // 2])
    assert ctx.expire_mlat_tracks(-inf) == 0 and store(ctx).tobytes() == got.tobytes()
    removed = ctx.expire_mlat_tracks(cut)               # last_ts == cutoff is kept
    assert removed == R.expire(tracks, cut) == (got["last_ts"] < cut).sum() > 0
    assert store(ctx).tobytes() == R.rows(tracks, ROW).tobytes() and (store(ctx)["last_ts"] >= cut).all()
    # a later call starts the expired addresses afresh and finds the kept ones stale
    s = ctx.stream_mlat_track(r, N.mlat_track_rule())
    exp = R.update(tracks, fixes, aux, {})
    assert s == exp and s["started"] >= removed and store(ctx).tobytes() == R.rows(tracks, ROW).tobytes()
    # the store is not decoder state
    kept = store(ctx)
    assert ctx.lib.adsb_streams_decoder_reset(ctx._h) == 0
    ctx.reset_stream(0)
    ctx.reset()
    assert store(ctx).tobytes() == kept.tobytes() and ctx.stream_dedup_stats()[1] == 0      # the carry is gone, the tracks are not
    assert ctx.expire_mlat_tracks(inf) == len(kept) and len(store(ctx)) == 0
    ctx.stream_mlat_track(r, N.mlat_track_rule())
    ctx.reset_mlat_tracks()
    assert len(store(ctx)) == 0
    G.push(ctx, G.sources(), G.CUTS_WHOLE)
    assert ctx.stream_mlat_track(r, N.mlat_track_rule())["tracks"] > 0
    ctx.close_streams()
    ctx.open_streams(G.N_RX)
    assert len(store(ctx)) == 0
    ctx.close()


def test_the_argument_table(pushed):
    """every refusal names the entry point, changes no track and writes nothing"""
    ctx = pushed
    ctx.stream_mlat_track(rule(), N.mlat_track_rule())
    before, dig = store(ctx), G.digest(ctx)
    nan = float("nan")
    st = N.MLAT_TRACK_STATS()
    ctypes.memset(ctypes.byref(st), 0xA5, ctypes.sizeof(st))

    def track(r=rule(), tr=N.mlat_track_rule(), t_lo=-inf, t_hi=inf):
        return ctx.lib.adsb_stream_mlat_track(ctx._h, t_lo, t_hi, ctypes.byref(r) if r is not None else None, ctypes.byref(tr) if tr is not None else None,
                                              ctypes.byref(st))

    def trk(**kw):
        reserved = kw.pop("reserved", 0)
        t = N.mlat_track_rule(**kw)
        t.reserved = reserved
        return t

    gains, bounds = "alpha and beta are finite and in (0, 1]", "gate_m, max_speed_mps and max_gap_s are finite and >= 0"
    cases = [(lambda: track(r=None), "rule is NULL"), (lambda: track(r=rule(solver=2)), "unknown solver"), (lambda: track(r=rule(flags=4)), "unknown flags"),
             (lambda: track(r=rule(GN, RESTART)), "flags need ADSB_MLAT_SOLVER_LM"), (lambda: track(r=rule(reserved=7)), "reserved is not 0"),
             (lambda: track(r=rule(min_rx=3)), "min_rx < 4 (< 3 with ADSB_MLAT_ALTITUDE)"),
             (lambda: track(r=rule(flags=N.MLAT_ALTITUDE, alt_weight=nan)), "alt_weight is not finite and > 0"),
             (lambda: track(t_lo=nan), "a bound is NaN"), (lambda: track(t_hi=nan), "a bound is NaN"),
             (lambda: track(tr=None), "track_rule is NULL"),
             (lambda: track(tr=trk(alpha=0.0)), gains), (lambda: track(tr=trk(alpha=1.0001)), gains), (lambda: track(tr=trk(alpha=nan)), gains),
             (lambda: track(tr=trk(beta=0.0)), gains), (lambda: track(tr=trk(beta=inf)), gains), (lambda: track(tr=trk(beta=-0.1)), gains),
             (lambda: track(tr=trk(gate_m=-1.0)), bounds), (lambda: track(tr=trk(gate_m=inf)), bounds), (lambda: track(tr=trk(max_speed_mps=nan)), bounds),
             (lambda: track(tr=trk(max_speed_mps=-1.0)), bounds), (lambda: track(tr=trk(max_gap_s=-1.0)), bounds), (lambda: track(tr=trk(max_gap_s=inf)), bounds),
             (lambda: track(tr=trk(max_rms_m=nan)), "max_rms_m or min_up_m is NaN"), (lambda: track(tr=trk(min_up_m=nan)), "max_rms_m or min_up_m is NaN"),
             (lambda: track(tr=trk(restart_after=0)), "restart_after < 1"), (lambda: track(tr=trk(reserved=1)), "track_rule->reserved is not 0")]
    for call, what in cases:
        assert call() == -EINVAL, what
        assert ctx.lib.adsb_last_error(ctx._h).decode() == "adsb_stream_mlat_track: " + what
        assert bytes(st) == b"\xA5" * 64 and store(ctx).tobytes() == before.tobytes()
    assert track(tr=trk(alpha=1.0, beta=1.0, gate_m=0.0, max_speed_mps=0.0, max_gap_s=0.0, max_rms_m=inf, min_up_m=-inf, restart_after=1)) == 0
    assert ctx.lib.adsb_stream_mlat_track(ctx._h, -inf, inf, ctypes.byref(rule()), ctypes.byref(N.mlat_track_rule()), None) == 0      # stats may be NULL
    assert store(ctx).tobytes() == before.tobytes() and G.digest(ctx) == dig
    # the readout: the count query, -ENOSPC writing nothing, the missing arguments
    n = ctypes.c_int32(-1)
    rows = np.frombuffer(bytearray(b"\xA5" * (len(before) + 2) * ROW.itemsize), dtype=ROW)
    read = lambda buf, cap, cutoff=-inf, np_=ctypes.byref(n): ctx.lib.adsb_stream_mlat_tracks(ctx._h, 1, cutoff, buf, cap, np_)      # noqa: E731
    assert read(None, 0) == -ENOSPC and n.value == len(before)
    assert read(rows.ctypes.data, len(before) - 1) == -ENOSPC and n.value == len(before) and (rows.view(np.uint8) == 0xA5).all()
    assert ctx.lib.adsb_last_error(ctx._h).decode() == "adsb_stream_mlat_tracks: cap is too small (*n)"
    assert read(rows.ctypes.data, len(before)) == 0 and rows[:len(before)].tobytes() == before.tobytes() and (rows[len(before):].view(np.uint8) == 0xA5).all()
    for call in (lambda: read(None, 1), lambda: read(rows.ctypes.data, -1), lambda: read(rows.ctypes.data, 4, np_=None), lambda: read(rows.ctypes.data, 4, nan)):
        assert call() == -EINVAL and ctx.lib.adsb_last_error(ctx._h).decode().startswith("adsb_stream_mlat_tracks: ")
    assert ctx.lib.adsb_stream_mlat_tracks_expire(ctx._h, nan, None) == -EINVAL
    assert ctx.lib.adsb_last_error(ctx._h).decode() == "adsb_stream_mlat_tracks_expire: cutoff is NaN"
    assert ctx.lib.adsb_stream_mlat_tracks_expire(ctx._h, -inf, None) == 0 and store(ctx).tobytes() == before.tobytes()
    ctx.reset_mlat_tracks()
    # without streams, and without the flag
    c2 = N.Context(G.FS, G.THR, flags=G.SD | G.SH | G.DD)
    k = ctypes.c_int64(0)
    for api, call in (("adsb_stream_mlat_track", lambda: c2.lib.adsb_stream_mlat_track(c2._h, -inf, inf, ctypes.byref(rule()), ctypes.byref(N.mlat_track_rule()), None)),
                      ("adsb_stream_mlat_tracks", lambda: c2.lib.adsb_stream_mlat_tracks(c2._h, 1, -inf, None, 0, ctypes.byref(n))),
                      ("adsb_stream_mlat_tracks_expire", lambda: c2.lib.adsb_stream_mlat_tracks_expire(c2._h, 0.0, ctypes.byref(k))),
                      ("adsb_stream_mlat_tracks_reset", lambda: c2.lib.adsb_stream_mlat_tracks_reset(c2._h))):
        assert call() == -EINVAL and c2.lib.adsb_last_error(c2._h).decode() == api + ": no streams (adsb_streams_open first)"
    c2.close()
    c3 = N.Context(G.FS, G.THR, flags=G.SD | G.SH)
    c3.open_streams(2)
    assert c3.lib.adsb_stream_mlat_tracks_reset(c3._h) == -EINVAL
    assert c3.lib.adsb_last_error(c3._h).decode() == "context created without ADSB_FLAG_STREAM_DEDUP"
    c3.close()


def test_the_front_end(native):      # noqa: F811
    """Receivers.track() / tracks(): latitude and longitude are ecef_to_geodetic's for the row; merged(mlat=True) points every
    extended-squitter aircraft at its own track; merged() and table() without the argument are what they were before the track
    calls."""
    fe = frontend.FrontEnd(G.FS, G.THR, flags=G.SD | G.SH | G.DD | G.AGES)
    rx = fe.receivers(G.N_RX, fmt=N.FMT_FC32, starts=G.STARTS, ages=True, shared=True, dedup=True, positions=G.LLA)
    rx.push([G.sources()[0]] * G.N_RX)
    rx.finish()
    rows0, info0 = rx.merged()
    table0 = rx.table(G.T0)
    stats = rx.track()
    assert stats["taken"] > 100 and stats["tracks"] >= 12
    assert stats == {**stats, **dict(stale=0, rejected=0)}
    t = rx.tracks()
    assert len(t) == 12 and (t["n_fixes"] >= 3).all() and len(rx.tracks(min_fixes=1)) == stats["tracks"]
    for r in t:
        la, lo, al = N.ecef_to_geodetic(r["x"], r["y"], r["z"])
        assert abs(r["latitude"] - la) <= 1e-6 and abs(r["longitude"] - lo) <= 1e-6 and abs(r["altitude_m"] - al) <= 1e-3
    assert np.abs(t["latitude"] - G.AIRCRAFT_LLA[0]).max() < 1e-4 and np.abs(t["longitude"] - G.AIRCRAFT_LLA[1]).max() < 1e-4
    assert (t["speed_kt"] < 100.0).all() and ((t["heading_deg"] >= 0) & (t["heading_deg"] < 360)).all()
    rows, info, track_of, tracks = rx.merged(mlat=True)
    assert rows.tobytes() == rows0.tobytes() and info.tobytes() == info0.tobytes() and len(track_of) == len(rows)
    es = (rows["icao"] >= 0x4B1A00) & (rows["icao"] < 0x4B1A00 + 12)
    assert es.sum() == 12 and (track_of[es] >= 0).all() and np.array_equal(tracks["icao"][track_of[es]], rows["icao"][es])
    assert all(tracks["icao"][k] == rows["icao"][j] for j, k in enumerate(track_of) if k >= 0)
    assert all(rows["icao"][j] not in tracks["icao"] for j, k in enumerate(track_of) if k < 0)
    again, info1 = rx.merged()
    assert again.tobytes() == rows0.tobytes() and info1.tobytes() == info0.tobytes() and rx.table(G.T0) == table0
    with_tracks = rx.table(G.T0, mlat=True)
    assert len(with_tracks) == len(table0)
    for j, (a, b) in enumerate(zip(table0, with_tracks)):
        if np.isnan(rows["latitude"][j]) and track_of[j] >= 0:
            assert a != b and "%11.7f" % tracks["latitude"][track_of[j]] in b
        else:
            assert a == b
    assert rx.track(solver="gauss-newton")["stale"] > 100           # the same heads, by the other solver: nothing newer
    assert rx.expire_tracks(inf) == stats["tracks"] and len(rx.tracks(min_fixes=1)) == 0
    rx.track(gate_m=5000.0, restart_after=2)
    rx.reset_tracks()
    assert len(rx.tracks(min_fixes=1)) == 0
    with pytest.raises(TypeError):
        rx.track(gain=1.0)
    with pytest.raises(ValueError):
        rx.track(solver="newton")
    rx.close()
