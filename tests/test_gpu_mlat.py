"""adsb_stream_mlat on the MI355X, through the C ABI: six receivers hear one aircraft's replies, the shared decoder's
de-duplication carry keeps every hearing, and adsb_mlat.hip groups and solves them.  Structure and positions equal
tests/mlat_replay.py -- the header's MULTILATERATION rule in plain Python -- fed the DELIVERED records' (stream, offset, bits,
flags) and the streams' starts, with test_mlat.py's rule and tolerance (TOL there: 2e-3 m, from the oracle's own
float64-vs-longdouble sensitivity); every fix lies within TOL plus the oracle's own distance of the aircraft.  The call changes
nothing a caller can see.  The CPU half (emulated kernels, every seam) is tests/test_mlat.py."""
import ctypes

import numpy as np
import pytest

import mlat_replay as MR
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from gr_adsb_amd import modulator as M
from test_mlat import SENS, TOL, compare

pytestmark = pytest.mark.gpu

F, SD, SH, DD, AGES = N.FLAG_FEC_CONSERVATIVE, N.FLAG_STREAM_DECODE, N.FLAG_STREAM_DECODE_SHARED, N.FLAG_STREAM_DEDUP, N.FLAG_PLANE_AGES
ENOSPC, EINVAL = 28, 22
FS = 2e6
THR = 0.05
T0 = 1000.0                        # a session epoch: the ulp of an arrival time is 0.1 ps (the header's PRECISION)
SLOT = 400                         # samples between replies: 200 us
N_REPLIES = 150
N_RX = 6
WINDOW = 0.002                     # the default
AIRCRAFT_LLA = (52.2, 4.7, 9000.0)
P = MR.geodetic_to_ecef(*AIRCRAFT_LLA)


def receivers_lla():
    """six antennas over about 200 km x 200 km, 0 .. 2500 m up: a geometry at which the oracle alone converges to the aircraft
    with all six and with the first five (found on the CPU with tests/mlat_replay.py; asserted by compare(converge=True))"""
    rng = np.random.default_rng(90)
    return [(52.0 + rng.uniform(-0.9, 0.9), 5.0 + rng.uniform(-1.45, 1.45), rng.uniform(0.0, 2500.0)) for _ in range(N_RX)]


LLA = receivers_lla()
RX = {s: tuple(MR.geodetic_to_ecef(*LLA[s])) for s in range(N_RX)}
STARTS = [T0 + float(np.sqrt(((P - np.array(RX[s])) ** 2).sum())) / MR.C for s in range(N_RX)]


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


_src = {}


def replies():
    """[150, 14]: extended squitters of 12 aircraft with random, distinct message fields (the receivers' delays reach 0.7 ms,
    more than the 200 us between replies: only distinct payloads keep the hearings of different replies apart), and every
    tenth reply a short one: DF 4, 5 and 11 in turn"""
    if "bits" not in _src:
        rng = np.random.default_rng(77)
        rows = []
        for k in range(N_REPLIES):
            f = np.zeros(112, np.uint8)
            if k % 10 == 9:
                df = (4, 5, 11)[(k // 10) % 3]
                f[:5] = [(df >> (4 - i)) & 1 for i in range(5)]
                f[5:56] = rng.integers(0, 2, 51)
            else:
                aa = 0x4B1A00 + k % 12
                f[:5], f[5:8] = [1, 0, 0, 0, 1], [1, 0, 1]
                f[8:32] = [(aa >> (23 - i)) & 1 for i in range(24)]
                f[32:37] = [(11 >> (4 - i)) & 1 for i in range(5)]
                f[37:88] = rng.integers(0, 2, 51)
                crc = M.crc24(f[:88])
                f[88:] = [(crc >> (23 - i)) & 1 for i in range(24)]
            rows.append(np.packbits(f))
        b = np.array(rows, np.uint8)
        assert len(set(r.tobytes() for r in b)) == N_REPLIES
        _src["bits"] = b
    return _src["bits"]


def iq_of(bits14, seed):
    """complex64 IQ of the rows one after another, 200 us apart (amplitude 1 over AWGN at -40 dB): about 2^16 samples"""
    sps = int(FS // 1e6)
    rows = np.unpackbits(bits14, axis=1)[:, :112]
    starts = 200 * sps + SLOT * np.arange(len(rows))
    rng = np.random.default_rng(seed)
    n = int(starts[-1] + SLOT + 400 * sps)
    z = ((rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) * np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
    for s, b in zip(starts, rows):
        env = M.burst_waveform(b, sps)
        z[s:s + len(env)] += env
    assert 1 << 15 < n < 1 << 17
    return z


FLIPPED = list(range(3, N_REPLIES, 20))            # the replies receiver 1 hears with one wrong bit (extended squitters all)


def sources():
    """Six receivers, ONE IQ source: every reply is heard at the same sample offset by all, so its arrival times differ by the
    starts alone.  Receiver 1 has a source of its own kind: the same replies, one flipped bit in a few of them."""
    if "iq" not in _src:
        b = replies()
        flipped = b.copy()
        flipped[FLIPPED, 6] ^= 0x08
        common = iq_of(b, 5)
        _src["iq"] = [common, iq_of(flipped, 5)] + [common] * (N_RX - 2)
    return _src["iq"]


def mlat_ctx(corr="Conservative", starts=STARTS, extra=0, positions=range(N_RX)):
    c = N.Context(FS, THR, flags=SD | SH | DD | extra | (F if corr == "Conservative" else 0))
    c.open_streams(N_RX)
    c.set_streams_decoder("All Messages")
    for s, t in enumerate(starts):
        c.set_stream_start(s, t)
    for s in positions:
        c.set_stream_ecef(s, *RX[s])
    return c


def push(ctx, srcs, cuts, device=False):
    """Every stream's samples in len(cuts[0]) + 1 calls cut at cuts[s], in a different item order each call, then an END call
    -> the delivered (stream, record) pairs of all calls"""
    fmt = N.FMT_FC32
    bases = []
    if device:
        for s in srcs:
            d = ctx.device_alloc(max(s.nbytes, 16))
            ctx.device_upload(d, np.ascontiguousarray(s))
            bases.append(d)
    got = []
    edges = [[0] + list(c) + [len(srcs[s])] for s, c in enumerate(cuts)]
    for k in range(len(edges[0]) - 1):
        ids = [int(i) for i in np.random.default_rng(k).permutation(N_RX)]
        spans = [(edges[i][k], edges[i][k + 1]) for i in ids]
        if device:
            r, first = ctx.process_stream_batch_device(fmt, ids, [bases[i] + lo * 8 for i, (lo, _) in zip(ids, spans)], [hi - lo for lo, hi in spans])
        else:
            r, first = ctx.process_stream_batch(fmt, ids, [srcs[i][lo:hi] for i, (lo, hi) in zip(ids, spans)])
        got += [(ids[j], r[t]) for j in range(len(ids)) for t in range(first[j], first[j + 1])]
    ids = list(range(N_RX))
    r, first = ctx.process_stream_batch(fmt, ids, [srcs[i][:0] for i in ids], end=True)
    got += [(ids[j], r[t]) for j in range(len(ids)) for t in range(first[j], first[j + 1])]
    for d in bases:
        ctx.device_free(d)
    return got


def carry_of(delivered, starts):
    """The carry the header describes, from the delivered records: ts = start + (double)offset / fs, ascending (no two are
    equal here), a record's payload its bits at the length ADSB_BURST_LONG says, None without ADSB_BURST_DEMOD"""
    rows = []
    for s, rec in delivered:
        ts = starts[s] + float(int(rec["offset"])) / FS
        part = bool(int(rec["flags"]) & N.BURST_DEMOD)
        rows.append((ts, MR.payload_of(rec["bits"], bool(int(rec["flags"]) & N.BURST_LONG)) if part else None, s))
    rows.sort(key=lambda r: r[0])
    assert len(set(r[0] for r in rows)) == len(rows)
    return rows


def digest(ctx):
    """everything a caller can see of the decoder and the carry"""
    rows, first = ctx.stream_planes()
    return (ctx.last_stream_decoded().tobytes(), ctx.last_stream_order().tobytes(), ctx.last_stream_duplicates().tobytes(),
            ctx.stream_dedup_stats(), ctx.stream_decoder_stats(), rows.tobytes(), first.tobytes(), [ctx.stream_state(i) for i in range(N_RX)])


CUTS_WHOLE = [[] for _ in range(N_RX)]
CUTS_THREE = [[9000 + 1700 * s, 41000 - 2300 * s] for s in range(N_RX)]


def oracle(delivered, starts, rx, **kw):
    lst = carry_of(delivered, starts)
    exp, ems, emt = MR.mlat(lst, WINDOW, rx, **kw)
    ld = MR.mlat(lst, WINDOW, rx, ft=np.longdouble, **kw)[0]
    return lst, exp, ems, emt, ld


@pytest.mark.parametrize("name,cuts,device", [("whole", CUTS_WHOLE, False), ("three", CUTS_THREE, False), ("device", CUTS_THREE, True)])
def test_six_receivers_locate_every_reply(native, name, cuts, device):
    """Every reply of the source is a six-hearing group at the aircraft, under two call partitions and through the device entry
    point: structure exact and positions within TOL of the replay, every fix within TOL (+ the oracle's own distance) of the
    aircraft, a repaired hearing in the group of the clean ones, and the state's digest unchanged by the call."""
    ctx = mlat_ctx()
    delivered = push(ctx, sources(), cuts, device)
    before = digest(ctx)
    fixes, ms, mt = ctx.stream_mlat()
    assert digest(ctx) == before
    again = ctx.stream_mlat(cap=len(fixes), member_cap=len(ms))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (fixes, ms, mt)))
    lst, exp, ems, emt, ld = oracle(delivered, STARTS, RX)
    compare(name, fixes, ms, mt, exp, ems, emt, truth=P, exp_ld=ld, converge=True)
    assert len(fixes) >= N_REPLIES - 2 and (fixes["status"] == N.MLAT_OK).all()
    # the replies receiver 1 heard with a wrong bit: where the Conservative rule repairs the hearing (it does for some of
    # them), the record carries ADSB_BURST_FEC_FIXED and lies in the group of the clean hearings; where it does not, the group
    # has the five clean ones and receiver 1's hearing, alone with its payload, gives no fix
    clean = set(r.tobytes() for r in replies())
    fixed = [rec for s, rec in delivered if s == 1 and int(rec["flags"]) & N.BURST_FEC_FIXED and rec["bits"].tobytes() in clean]
    repaired = set(rec["bits"].tobytes() for rec in fixed) & set(replies()[FLIPPED][k].tobytes() for k in range(len(FLIPPED)))
    assert 1 <= len(repaired) <= len(FLIPPED)
    short_of_one = np.array([f["bits"].tobytes() in set(r.tobytes() for r in replies()[FLIPPED]) - repaired for f in fixes])
    assert short_of_one.sum() == len(FLIPPED) - len(repaired)
    assert np.array_equal(fixes["n_rx"], np.where(short_of_one, N_RX - 1, N_RX)) and np.array_equal(fixes["n_heard"], fixes["n_rx"])
    assert (np.diff(fixes["ts"]) > 0).all() and np.array_equal(fixes["first"], np.cumsum(fixes["n_rx"]) - fixes["n_rx"])
    for pay in repaired:
        j = int(np.flatnonzero([f["bits"].tobytes() == pay for f in fixes])[0])
        assert 1 in ms[fixes["first"][j]:fixes["first"][j] + N_RX].tolist()
    p = np.stack([fixes["x"], fixes["y"], fixes["z"]], axis=1)
    own = max(float(np.sqrt(((e["p"] - P) ** 2).sum())) for e in exp)
    assert float(np.sqrt(((p - P) ** 2).sum(axis=1)).max()) <= TOL + own and own < 0.5
    assert np.abs(fixes["t_tx"] - (fixes["ts"] - (STARTS[int(ms[0])] - T0))).max() < 1e-9
    # the extended squitters announce their address, the short replies carry it under address/parity
    es = fixes["bits"][:, 0] >> 3 == 17
    assert es.sum() >= 130 and set(fixes["icao"][es].tolist()) == set(range(0x4B1A00, 0x4B1A0C)) and (fixes["flags"][es] == N.BURST_LONG).all()
    for f in fixes[~es]:
        df = int(f["bits"][0]) >> 3
        assert f["flags"] == 0 and not f["bits"][7:].any()
        assert f["icao"] == (int.from_bytes(f["bits"][1:4].tobytes(), "big") if df == 11 else N.mode_s_syndrome(f["bits"])[0])
    # the range and min_rx
    mid = float(fixes["ts"][len(fixes) // 2])
    lo_half, _, _ = ctx.stream_mlat(t_hi=mid)
    hi_half, hms, _ = ctx.stream_mlat(t_lo=mid, min_rx=N_RX)
    assert len(lo_half) == len(fixes) // 2 and lo_half.tobytes() == fixes[:len(lo_half)].tobytes()
    assert np.array_equal(hi_half["ts"], fixes["ts"][len(lo_half):][fixes["n_rx"][len(lo_half):] == N_RX]) and hi_half["first"][0] == 0
    assert len(hms) == N_RX * len(hi_half)
    assert len(ctx.stream_mlat(min_rx=N_RX + 1)[0]) == 0
    k, ulp_m = ctx.stream_mlat_stats()
    assert k == N_RX and ulp_m == MR.C * np.spacing(ctx.stream_dedup_stats()[2]) and ulp_m < 1e-4
    assert digest(ctx) == before
    _src[name] = (fixes.copy(), ms.copy(), mt.copy())
    if name != "whole" and "whole" in _src:                            # the partition is not seen: the carry is the same
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_src[name], _src["whole"]))
    ctx.close()


def test_a_receiver_beyond_the_window_and_one_without_a_position(native):
    """Receiver 5 is 10 ms late, beyond the window: the groups have five hearings, and its own hearings -- heads of groups of
    one -- give no fix.  Without a position for receiver 4 the groups still count five hearings and use four."""
    starts = STARTS[:5] + [STARTS[5] + 0.01]
    ctx = mlat_ctx(corr="None", starts=starts)
    delivered = push(ctx, [sources()[0]] * N_RX, CUTS_THREE)
    fixes, ms, mt = ctx.stream_mlat()
    lst, exp, ems, emt, ld = oracle(delivered, starts, RX)
    compare("late", fixes, ms, mt, exp, ems, emt, truth=P, exp_ld=ld, converge=True)
    assert len(fixes) >= N_REPLIES - 2 and (fixes["n_rx"] == 5).all() and (fixes["n_heard"] == 5).all() and 5 not in ms.tolist()
    heads = [h for h, _ in MR.groups(lst, WINDOW)]
    assert len(heads) == 2 * len(fixes)                                 # the late hearings are heads, and nothing more
    ctx.close()
    ctx = mlat_ctx(corr="None", starts=starts, positions=range(4))
    assert ctx.stream_mlat_stats()[0] == 4
    delivered = push(ctx, [sources()[0]] * N_RX, CUTS_WHOLE)
    fixes, ms, mt = ctx.stream_mlat()
    rx4 = {s: RX[s] for s in range(4)}
    lst, exp, ems, emt, ld = oracle(delivered, starts, rx4)
    compare("four", fixes, ms, mt, exp, ems, emt, exp_ld=ld, converge=False)
    assert len(fixes) >= N_REPLIES - 2 and (fixes["n_rx"] == 4).all() and (fixes["n_heard"] == 5).all() and set(ms.tolist()) == {0, 1, 2, 3}
    assert len(ctx.stream_mlat(min_rx=5)[0]) == 0
    ctx.close()


def _code(fn, *a, **k):
    with pytest.raises(N.AdsbError) as e:
        fn(*a, **k)
    return e.value.code


def raw_mlat(ctx, cap, member_cap, t_lo=-np.inf, t_hi=np.inf, min_rx=4):
    """adsb_stream_mlat with buffers of exactly cap / member_cap entries and a guard entry behind each"""
    fixes = np.zeros(cap + 1, dtype=N.MLAT_DTYPE)
    fixes.view(np.uint8)[:] = 0xA5
    ms, mt = np.full(member_cap + 1, -77, np.int32), np.full(member_cap + 1, -77.0)
    n, m = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = ctx.lib.adsb_stream_mlat(ctx._h, t_lo, t_hi, min_rx, fixes.ctypes.data, cap, ctypes.byref(n), ms.ctypes.data, mt.ctypes.data, member_cap,
                                  ctypes.byref(m))
    return rc, n.value, m.value, fixes, ms, mt


def test_refusals_no_space_and_what_resets_keep(native):
    src = sources()[0]
    for flags in (SD | SH, SD, 0):                                     # a context without the flag
        c = N.Context(FS, THR, flags=flags)
        c.open_streams(2)
        assert _code(c.stream_mlat) == -EINVAL and _code(c.set_stream_ecef, 0, *RX[0]) == -EINVAL and _code(c.stream_mlat_stats) == -EINVAL
        c.close()
    ctx = N.Context(FS, THR, flags=SD | SH | DD)
    assert _code(ctx.stream_mlat) == -EINVAL and _code(ctx.set_stream_ecef, 0, *RX[0]) == -EINVAL      # no streams yet
    ctx.close()
    ctx = mlat_ctx(corr="None")
    assert ctx.stream_mlat()[0].shape == (0,) and raw_mlat(ctx, 0, 0)[:3] == (0, 0, 0)                  # an empty carry
    assert _code(ctx.stream_mlat, min_rx=3) == -EINVAL and _code(ctx.stream_mlat, min_rx=0) == -EINVAL
    assert _code(ctx.stream_mlat, t_lo=float("nan")) == -EINVAL and _code(ctx.stream_mlat, t_hi=float("nan")) == -EINVAL
    assert _code(ctx.set_stream_ecef, N_RX, *RX[0]) == -EINVAL and _code(ctx.set_stream_ecef, -1, *RX[0]) == -EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _code(ctx.set_stream_ecef, 0, RX[0][0], bad, RX[0][2]) == -EINVAL
    assert ctx.stream_mlat_stats()[0] == N_RX
    push(ctx, [src] * N_RX, CUTS_WHOLE)
    before = digest(ctx)
    rc, n, m, fixes, ms, mt = raw_mlat(ctx, 0, 0)                       # the count query
    assert rc == -ENOSPC and n >= N_REPLIES - 2 and m == N_RX * n
    for cap, member_cap in ((n - 1, m), (n, m - 1)):                   # one short, either way: the counts, and nothing written
        rc, n2, m2, fixes, ms, mt = raw_mlat(ctx, cap, member_cap)
        assert rc == -ENOSPC and (n2, m2) == (n, m)
        assert (fixes.view(np.uint8) == 0xA5).all() and (ms == -77).all() and (mt == -77.0).all()
    rc, n2, m2, fixes, ms, mt = raw_mlat(ctx, n, m)
    assert rc == 0 and (n2, m2) == (n, m) and (fixes[n:].view(np.uint8) == 0xA5).all() and ms[m] == -77 and mt[m] == -77.0
    assert (fixes["status"][:n] == N.MLAT_OK).all() and digest(ctx) == before
    full = ctx.stream_mlat(cap=1, member_cap=1)                        # the Python call asks again with what is needed
    assert full[0].tobytes() == fixes[:n].tobytes() and full[1].tobytes() == ms[:m].tobytes()
    assert raw_mlat(ctx, 0, 0, t_lo=2000.0)[:3] == (0, 0, 0) and raw_mlat(ctx, 0, 0, t_lo=1000.01, t_hi=1000.0)[:3] == (0, 0, 0)      # empty ranges
    # the positions are not decoder state
    ctx.reset_stream(0)
    assert ctx.stream_mlat_stats()[0] == N_RX and len(ctx.stream_mlat()[0]) == n
    ctx.reset_streams_decoder()
    assert ctx.stream_mlat_stats()[0] == N_RX and ctx.stream_mlat()[0].shape == (0,)
    ctx.reset()
    assert ctx.stream_mlat_stats()[0] == N_RX
    ctx.close_streams()
    ctx.open_streams(N_RX)
    assert ctx.stream_mlat_stats() == (0, MR.C * 5e-324)
    ctx.close()


def test_the_front_end(native):
    """FrontEnd.receivers(positions=...) and Receivers.mlat(): latitude, longitude and altitude of the aircraft; None opens a
    side of the range; ValueError without dedup."""
    fe = frontend.FrontEnd(FS, THR, flags=SD | SH | DD)
    rx = fe.receivers(N_RX, fmt=N.FMT_FC32, starts=STARTS, shared=True, dedup=True, positions=LLA)
    assert fe.ctx.stream_mlat_stats()[0] == N_RX
    rx.push([sources()[0]] * N_RX)
    rx.finish()
    fixes, ms, mt = rx.mlat()
    assert len(fixes) >= N_REPLIES - 2 and (fixes["status"] == N.MLAT_OK).all() and (fixes["n_rx"] == N_RX).all()
    # the receivers' ECEF came through adsb_geodetic_to_ecef instead of the oracle's: millimetres at the most
    assert np.abs(fixes["latitude"] - AIRCRAFT_LLA[0]).max() < 1e-6 and np.abs(fixes["longitude"] - AIRCRAFT_LLA[1]).max() < 1e-6
    assert np.abs(fixes["altitude_m"] - AIRCRAFT_LLA[2]).max() < 0.1
    mid = float(fixes["ts"][40])
    assert len(rx.mlat(t_hi=mid)[0]) == 40 and len(rx.mlat(t_lo=mid)[0]) == len(fixes) - 40 and len(rx.mlat(min_rx=7)[0]) == 0
    rx.close()
    fe.ctx.close()
    with pytest.raises(ValueError):
        frontend.FrontEnd(FS, THR, flags=SD | SH).receivers(N_RX, shared=True, positions=LLA)
    fe = frontend.FrontEnd(FS, THR, flags=SD | SH | DD)
    rx = fe.receivers(2, shared=True, dedup=True, positions=[LLA[0], None])
    assert fe.ctx.stream_mlat_stats()[0] == 1
    rx.close()
    fe.ctx.close()
    assert SENS <= TOL / 16
