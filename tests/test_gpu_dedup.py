"""ADSB_FLAG_STREAM_DEDUP on the MI355X, through the C ABI: receivers that hear the same replies feed one shared decoder, and a
reply is published once (adsb_dedup.hip inside fleet_step).  Every call's records, rows, order[], dup[] and the stats equal
tests/dedup_replay.py -- the header's rule in plain Python around one decoder -- over the records of a context without any
decoder.  The carry across random chunkings and a short horizon, a repaired hearing, a fallback item, the refusals, a refused
call, the resets, and the contexts beside it, unchanged.  The CPU half (emulator, the reference's golden) is
tests/test_dedup.py."""
import numpy as np
import pytest

import decode_streams as S
import dedup_replay as DR
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from test_gpu_decode import THR, stream
from test_gpu_shared_decode import AP_BITS, Expect, check, ctx_of, plain_run, run, schedule
from test_gpu_stream_decode import _code, cat, sparse_mag2
from test_stream_decode import ISO_ADDR

pytestmark = pytest.mark.gpu

F, SD, SH, DD, AGES = N.FLAG_FEC_CONSERVATIVE, N.FLAG_STREAM_DECODE, N.FLAG_STREAM_DECODE_SHARED, N.FLAG_STREAM_DEDUP, N.FLAG_PLANE_AGES
ENOSPC, EINVAL = 28, 22
FS = 2e6
T0 = 1760000000.625
# bursts are 200 us apart, so a window of 100 us matches hearings of one slot only.  Receivers 1 and 2 hear everything 40 and
# 80 us after receiver 0 (below the window), receiver 3 150 us after it (above the window from 0 and 1, below it from 2: its
# hearings are duplicates of duplicates), receiver 4 10 ms later (above it from everybody: published again)
WINDOW = 1e-4
DELAYS = [0.0, 40e-6, 80e-6, 150e-6, 0.01]
STARTS = [T0 + d for d in DELAYS]


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


_src = {}


def shared_bits():
    """[5] x [250, 14]: the same 250 replies of 20 aircraft as each receiver slices them -- its own noise behind a short
    reply, and on receiver 1 one flipped bit in every fifth extended squitter"""
    if "bits" not in _src:
        common, _ = S.mixed(np.random.default_rng(900), n=250, addresses=ISO_ADDR[:20], t0=0.0, dt=(0.002, 0.05))
        out = []
        for s in range(5):
            b = common.copy()
            short = np.isin(b[:, 0] >> 3, (0, 4, 5, 11))
            b[short, 7:] = np.random.default_rng(910 + s).integers(0, 256, (int(short.sum()), 7))
            if s == 1:
                es = np.flatnonzero((b[:, 0] >> 3) == 17)[::5]
                b[es, 5] ^= 0x10
            out.append(b)
        _src["bits"] = out
    return _src["bits"]


SLOTS = 250


def flipped_slots():
    """the slots in which receiver 1 hears one wrong bit"""
    return len(np.flatnonzero((shared_bits()[0][:, 0] >> 3) == 17)[::5])


def fleet_sources(fmt):
    """Five receivers of about 2^16.6 samples each that hear the same replies in the same slots"""
    if fmt not in _src:
        from gr_adsb_amd import modulator as M
        out = []
        for b in shared_bits():
            iq, _ = stream(b, FS)
            assert 1 << 16 <= len(iq) <= 1 << 17
            out.append(iq if fmt == N.FMT_FC32 else M.quantize_iq8(iq, offset_binary=True))
        _src[fmt] = out
    return _src[fmt]


def dedup_ctx(filt, corr, n_streams, starts, window=WINDOW, horizon=1.0, extra=0):
    c = ctx_of(SD | SH | DD | extra, filt, corr, n_streams, starts)
    if window is not None:
        c.set_streams_dedup(window, horizon)
    return c


class ExpectDedup:
    """dedup_replay.Replay over delivered records: a payload is the record's bits at the length its ADSB_BURST_LONG says."""

    def __init__(self, filt, corr, starts, window=WINDOW, horizon=1.0):
        self.rep, self.starts = DR.Replay(filt, corr, window, horizon), starts

    def call(self, recs, first, ids):
        """recs: the call's records without verdict flags -> (records with them, rows, order, dup)"""
        n = len(recs)
        stream_of = np.repeat(np.asarray(ids, np.int64), np.diff(np.asarray(first[:len(ids) + 1], np.int64)))
        ts = np.array([self.starts[int(s)] + int(o) / FS for s, o in zip(stream_of, recs["offset"])], np.float64)
        dem = (recs["flags"] & N.BURST_DEMOD) != 0
        pay = [DR.record_payload(recs[t]) if dem[t] else None for t in range(n)]
        flags, replayed, order, dup = self.rep.call(recs["bits"], ts, stream_of, dem=dem, pay=pay)
        want = recs.copy()
        want["flags"] |= flags
        rows = np.zeros(n, dtype=N.DECODED_DTYPE)              # a record without a PDU, and under port 4 a duplicate
        rows["icao"], rows["bits"], rows["df"] = -1, recs["bits"], recs["bits"][:, 0] >> 3
        rows["latitude"] = rows["longitude"] = np.nan
        rows["port"][dup != -1] = N.DEC_DUPLICATE
        pub = [t for t in range(n) if replayed[t] is not None]
        if pub:
            rows[pub] = S.to_rows([replayed[t] for t in pub])
        return want, rows, order.astype(np.int32), dup


def run_dedup(ctx, fmt, srcs, sched, device=False):
    """test_gpu_shared_decode.run, with dup[] and the stats after every call"""
    per, bps = N.FMT_LAYOUT[fmt][1], N.FMT_BYTES[fmt]
    bases = []
    if device:
        for s in srcs:
            b = ctx.device_alloc(max(s.nbytes, 16))
            ctx.device_upload(b, np.ascontiguousarray(s))
            bases.append(b)
    out = []
    for ids, spans, end in sched:
        if device and not end:
            r, first = ctx.process_stream_batch_device(fmt, ids, [bases[i] + lo * bps for i, (lo, _) in zip(ids, spans)],
                                                       [hi - lo for lo, hi in spans])
        else:
            r, first = ctx.process_stream_batch(fmt, ids, [srcs[i][lo * per:hi * per] for i, (lo, hi) in zip(ids, spans)], end=end)
        out.append((ids, r, first.copy(), ctx.last_stream_decoded(), ctx.last_stream_order(), ctx.last_stream_duplicates(),
                    ctx.stream_dedup_stats()))
    for b in bases:
        ctx.device_free(b)
    return out


def check_dedup(got, plain, exp):
    tally = dict(records=0, duplicates=0, earlier=0, fixed_dups=0, decoded=0)
    for (ids, r, first, rows, order, dup, stats), (_, pr, pfirst, _, _) in zip(got, plain):
        assert list(first) == list(pfirst) and len(r) == len(pr) == len(rows) == len(order) == len(dup) == first[len(ids)]
        want, wrows, worder, wdup = exp.call(pr, first, ids)
        assert np.array_equal(order, worder)
        assert np.array_equal(dup, wdup), (np.flatnonzero(dup != wdup)[:5], dup[dup != wdup][:5], wdup[dup != wdup][:5])
        assert r.tobytes() == want.tobytes()
        assert r["flags"][dup != -1].tobytes() == pr["flags"][dup != -1].tobytes()      # a context without a decoder's
        if len(r):
            S.assert_rows_equal(rows, wrows)
        assert stats == exp.rep.stats()
        tally["records"] += len(r)
        tally["duplicates"] += int((dup != -1).sum())
        tally["earlier"] += int((dup == -2).sum())
        tally["fixed_dups"] += int(((dup != -1) & ((r["flags"] & N.BURST_FEC_FIXED) != 0)).sum())
        tally["decoded"] += int((rows["port"] == N.DEC_DECODED).sum())
    return tally


# ---- 1. records, rows, order, dup and stats equal the rule around one decoder ---------------------------------------------
@pytest.mark.parametrize("fmt_name,corr,horizon", [("fc32", "None", 1.0), ("cu8", "Conservative", 1.0), ("cu8", "None", 0.004)])
def test_everything_equals_the_replay(native, fmt_name, corr, horizon):
    """Random chunks to random subsets in random item order, an n == 0 item and END items; fc32 through the host entry point,
    cu8 through the device one.  horizon = 4 ms: the receivers' deliveries lag more than that, so the carry forgets hearings
    and the replay says which are published again.  On the Conservative context a hearing with one flipped bit, where it
    carries ADSB_BURST_FEC_FIXED, is a duplicate of the clean hearing."""
    fmt = {"fc32": N.FMT_FC32, "cu8": N.FMT_CU8}[fmt_name]
    filt = "All Messages"
    srcs = fleet_sources(fmt)
    sched = schedule(srcs, fmt, seed=81, hi=40000)
    ctx = dedup_ctx(filt, corr, 5, STARTS, horizon=horizon)
    got = run_dedup(ctx, fmt, srcs, sched, device=(fmt == N.FMT_CU8))
    exp = ExpectDedup(filt, corr, STARTS, horizon=horizon)
    t = check_dedup(got, plain_run(fmt, corr, srcs, sched, ("dedup", 81)), exp)
    print(t)
    assert t["records"] == 5 * SLOTS and t["earlier"] > 0 and t["duplicates"] - t["earlier"] > 0
    # Receivers 0, 1 and 2 lie pairwise within the window, so of their hearings of a slot exactly one is published, whoever
    # delivers first: two duplicates a slot -- one where receiver 1's flipped bit stays unrepaired.  Receiver 3 is within the
    # window of receiver 2 only: a duplicate iff 2's hearing is published before it, which the chunking decides.  Receiver 4
    # never is one.
    flipped = 0 if corr == "Conservative" else flipped_slots()
    held = 2 * (SLOTS - flipped) + flipped
    if horizon >= 1.0:
        assert held <= t["duplicates"] <= held + SLOTS
    else:                                                      # a carry that forgets can only lose matches, and here it does
        full = ExpectDedup(filt, corr, STARTS, horizon=1.0)
        n_full = sum(int((full.call(pr, first, ids)[3] != -1).sum()) for ids, pr, first, _, _ in plain_run(fmt, corr, srcs, sched, ("dedup", 81)))
        assert held <= n_full <= held + SLOTS and 0 < t["duplicates"] < n_full
    assert ctx.stream_decoder_stats()[0] == len(exp.rep.rep.dec.planes) >= 10
    ctx.close()


def test_a_fully_shared_aircraft_counts_as_for_one_receiver(native):
    """Receivers 0, 1 and 2 hear every reply within the window: every plane's num_msgs, and every other field, is what ONE
    receiver's shared decoder holds -- a third of what the fleet counts without the flag."""
    fmt, filt, corr = N.FMT_FC32, "All Messages", "None"
    srcs = fleet_sources(fmt)[:3]
    n = [len(s) for s in srcs]
    planes = {}
    for name, flags, k in (("dedup", SD | SH | DD, 3), ("one", SD | SH, 1), ("fleet", SD | SH, 3)):
        ctx = ctx_of(flags, filt, corr, k, STARTS[:k])
        if flags & DD:
            ctx.set_streams_dedup(WINDOW, 1.0)
        ids = list(range(k))[::-1]
        ctx.process_stream_batch(fmt, ids, [srcs[i] for i in ids])
        ctx.process_stream_batch(fmt, ids, [srcs[i][n[i]:] for i in ids], end=True)
        rows, _ = ctx.stream_planes()
        planes[name] = rows[np.argsort(rows["icao"])]
        if flags & DD:
            dups, carried, hi = ctx.stream_dedup_stats()      # receiver 0 is first in time: 1 and 2 are duplicates but for the flipped bits
            assert carried == 3 * SLOTS and dups == 2 * SLOTS - flipped_slots() and hi > T0
        ctx.close()
    assert len(planes["one"]) >= 10 and planes["dedup"].tobytes() == planes["one"].tobytes()
    # without the flag every hearing counts, but for receiver 1's flipped bits, which fail parity
    assert 3 * planes["one"]["num_msgs"].sum() - flipped_slots() <= planes["fleet"]["num_msgs"].sum() <= 3 * planes["one"]["num_msgs"].sum()


def test_a_repaired_hearing_is_a_duplicate_of_the_clean_one(native):
    """Conservative, the three receivers whole in one call: receiver 1's hearings with one flipped bit carry
    ADSB_BURST_FEC_FIXED, their payload is the repaired reply, and each is a duplicate of receiver 0's clean hearing."""
    fmt = N.FMT_FC32
    srcs = fleet_sources(fmt)[:3]
    ctx = dedup_ctx("All Messages", "Conservative", 3, STARTS[:3])
    r, first = ctx.process_stream_batch(fmt, [2, 1, 0], [srcs[i] for i in (2, 1, 0)])
    dup = ctx.last_stream_duplicates()
    fixed = np.flatnonzero((r["flags"] & N.BURST_FEC_FIXED) != 0)
    mine = fixed[(fixed >= first[1]) & (fixed < first[2])]                  # receiver 1's repaired hearings
    assert len(mine) > 0 and (dup[mine] >= first[2]).all()                    # each matches a hearing of receiver 0, in this call
    assert (r["flags"][mine] & N.BURST_DEMOD).all() and (ctx.last_stream_decoded()["port"][mine] == N.DEC_DUPLICATE).all()
    assert (r["bits"][mine] == r["bits"][dup[mine]]).all()
    clean = (r["flags"][dup[mine]] & N.BURST_FEC_FIXED) == 0                 # ... which receiver 0 heard without the error
    assert clean.sum() >= 1 and clean.sum() <= flipped_slots()
    ctx.close()


# ---- 2. the guarantees of a stream-batch call -----------------------------------------------------------------------------
def test_a_refused_call_changes_nothing(native):
    """-ENOSPC leaves the streams, the decoder, the carry, hi and the last call's dup[] alone; repeated with room, the same
    bytes as a run that was never refused."""
    fmt, filt, corr = N.FMT_FC32, "All Messages", "Conservative"
    srcs = fleet_sources(fmt)[:3]
    cuts_a, cuts_b = [30000, 50000, 20000], [70000, 60000, 90000]

    def grab(ctx, res):
        return res + (ctx.last_stream_decoded(), ctx.last_stream_order(), ctx.last_stream_duplicates(), ctx.stream_dedup_stats())

    def go(ctx, refuse):
        out = [grab(ctx, ctx.process_stream_batch(fmt, [1, 0, 2], [srcs[i][:cuts_a[i]] for i in (1, 0, 2)]))]
        mid = [srcs[i][cuts_a[i]:cuts_b[i]] for i in (0, 2, 1)]
        if refuse:
            before = [ctx.stream_state(i) for i in range(3)], ctx.stream_decoder_stats(), ctx.stream_dedup_stats()
            assert before[2][0] > 20 and before[2][1] > 100
            assert _code(ctx.process_stream_batch, fmt, [0, 2, 1], mid, cap=3) == -ENOSPC
            assert ([ctx.stream_state(i) for i in range(3)], ctx.stream_decoder_stats(), ctx.stream_dedup_stats()) == before
            assert np.array_equal(ctx.last_stream_duplicates(), out[0][4]) and np.array_equal(ctx.last_stream_order(), out[0][3])
        out.append(grab(ctx, ctx.process_stream_batch(fmt, [0, 2, 1], mid)))
        out.append(grab(ctx, ctx.process_stream_batch(fmt, [2, 1, 0], [srcs[i][cuts_b[i]:] for i in (2, 1, 0)], end=True)))
        return out

    a = go(dedup_ctx(filt, corr, 3, STARTS[:3]), True)
    b = go(dedup_ctx(filt, corr, 3, STARTS[:3]), False)
    for x, y in zip(a, b):
        assert x[0].tobytes() == y[0].tobytes() and list(x[1]) == list(y[1]) and x[2].tobytes() == y[2].tobytes()
        assert np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4]) and x[5] == y[5]
    assert sum(int((x[4] == -2).sum()) for x in a) > 50


def test_a_fallback_item_takes_part(native):
    """An item too long for the batch kernel takes the ordinary pass inside the call; its records are de-duplicated with the
    rest: receivers 1 and 2 hear the first 150 of its replies in the same samples."""
    filt, corr, fmt = "All Messages", "Conservative", N.FMT_MAG2
    b_long, _ = S.mixed(np.random.default_rng(61), n=400, addresses=ISO_ADDR[:12])
    srcs = [sparse_mag2(b_long, N.BATCH_ITEM_MAX + 4096, 10000, 1)]
    for s in (1, 2):
        srcs.append(sparse_mag2(b_long[:150], 150 * 10000 + 1000, 10000, 1 + s))
    starts = [T0, T0, T0 + 50e-6]
    sched = [([1, 0, 2], [(0, len(srcs[i])) for i in (1, 0, 2)], False), ([0, 1, 2], [(len(srcs[i]),) * 2 for i in range(3)], True)]
    ctx = dedup_ctx(filt, corr, 3, starts)
    out = []
    for ids, spans, end in sched:
        r, first = ctx.process_stream_batch(fmt, ids, [srcs[i][lo:hi] for i, (lo, hi) in zip(ids, spans)], end=end)
        if not end:
            assert ctx.last_batch_fallbacks == 1
        out.append((ids, r, first.copy(), ctx.last_stream_decoded(), ctx.last_stream_order(), ctx.last_stream_duplicates(),
                    ctx.stream_dedup_stats()))
    exp = ExpectDedup(filt, corr, starts, window=0.002)
    t = check_dedup(out, plain_run(fmt, corr, srcs, sched, "dedup_fallback"), exp)
    assert t["records"] >= 690 and 250 <= t["duplicates"] <= 300 and ctx.stream_decoder_stats()[0] == len(exp.rep.rep.dec.planes) >= 10
    ctx.close()


# ---- 3. entry points, refusals, resets -------------------------------------------------------------------------------------
def test_refusals(native):
    for flags in (DD, DD | SD, DD | SH, DD | SD | F, DD | SH | N.FLAG_DECODE | N.FLAG_AIRCRAFT_TABLE):
        with pytest.raises(N.AdsbError) as e:
            N.Context(FS, THR, flags=flags)
        assert e.value.code == -EINVAL
    ctx = N.Context(FS, THR, flags=SD | SH | DD | F | AGES)
    for fn in (ctx.set_streams_dedup, ctx.last_stream_duplicates, ctx.stream_dedup_stats):
        assert _code(fn) == -EINVAL                           # no streams yet
    ctx.open_streams(2)
    assert len(ctx.last_stream_duplicates()) == 0 and ctx.stream_dedup_stats() == (0, 0, 0.0)
    for w, h in ((float("nan"), 1.0), (0.002, float("nan")), (-1e-9, 1.0), (0.002, -1.0), (0.002, 0.001)):
        assert _code(ctx.set_streams_dedup, w, h) == -EINVAL
    ctx.set_streams_dedup(0.0, 0.0)
    ctx.set_streams_dedup(0.002, 0.002)
    ctx.set_streams_dedup()
    r, first = ctx.process_stream_batch(N.FMT_FC32, [], [])
    assert len(r) == 0 and len(ctx.last_stream_duplicates()) == 0
    ctx.set_streams_dedup(0.001, 2.0)                       # nothing has been delivered
    ctx.close_streams()
    assert _code(ctx.stream_dedup_stats) == -EINVAL
    ctx.close()
    for flags in (SD | SH, SD, 0):
        c = N.Context(FS, THR, flags=flags)
        c.open_streams(2)
        for fn in (c.set_streams_dedup, c.last_stream_duplicates, c.stream_dedup_stats):
            assert _code(fn) == -EINVAL
        c.close()
    with pytest.raises(ValueError):
        frontend.FrontEnd(FS, THR, flags=SD | SH).receivers(2, shared=True, dedup=True)
    with pytest.raises(ValueError):
        frontend.FrontEnd(FS, THR, flags=SD | SH | DD).receivers(2, shared=True)


def test_resets_and_the_front_end(native):
    """adsb_stream_reset and END items leave the carry alone, adsb_stream_planes_expire too; adsb_streams_decoder_reset and
    adsb_reset clear it, and only then may the window change again.  frontend.Receivers(dedup=(window, horizon)):
    .duplicates beside .order."""
    fmt = N.FMT_FC32
    srcs = [fleet_sources(fmt)[i] for i in (0, 2)]                         # (receiver 1's flipped bits need the repair to match)
    half = 40000
    fe = frontend.FrontEnd(FS, THR, flags=SD | SH | DD | AGES)
    rx = fe.receivers(2, fmt=fmt, starts=STARTS[:2], ages=True, shared=True, dedup=(WINDOW, 1.0))
    ctx = fe.ctx
    out = rx.push([srcs[0][:half]], ids=[0])
    n0 = len(out[0])
    assert n0 > 50 and (rx.duplicates == -1).all() and len(rx.duplicates) == len(rx.order) == n0
    assert _code(ctx.set_streams_dedup, 0.001, 1.0) == -EINVAL            # a call has been delivered
    assert ctx.stream_dedup_stats()[:2] == (0, n0)
    ctx.reset_stream(1)                                                    # framing only
    ctx.reset_stream(0)                                                    # ... also for index 0, under which the one decoder lives
    assert ctx.stream_state(0)[0] == 0 and len(rx.planes()) > 0
    rx.expire(0)
    assert ctx.stream_dedup_stats()[:2] == (0, n0)
    out = rx.push([srcs[1][:half]], ids=[1])                               # the other receiver's hearings of the same replies
    dem = (out[0]["flags"] & N.BURST_DEMOD) != 0
    assert len(out[0]) == n0 and (rx.duplicates[dem] == -2).all() and (rx.rows[0]["port"][dem] == N.DEC_DUPLICATE).all()
    assert ctx.stream_dedup_stats()[:2] == (int(dem.sum()), 2 * n0)
    rx.finish([1])                                                         # an END item: the carry stays
    assert ctx.stream_dedup_stats()[1] >= 2 * n0
    ctx.reset_streams_decoder()
    assert ctx.stream_dedup_stats() == (0, 0, 0.0) and len(rx.planes()) == 0
    ctx.set_streams_dedup(WINDOW, 1.0)                                     # fresh: allowed again
    out = rx.push([srcs[1][:half]], ids=[1])                               # nobody remembers receiver 0's hearings
    assert (rx.duplicates == -1).all() and (rx.rows[0]["port"] != N.DEC_DUPLICATE).all()
    ctx.reset()
    assert ctx.stream_dedup_stats() == (0, 0, 0.0)
    rx.close()
    ctx.close()


# ---- 4. the contexts beside it ---------------------------------------------------------------------------------------------
def test_one_stream_with_the_flag_and_a_fleet_without_it(native):
    """A context with the flag and ONE stream gives the bytes of a shared context without it and marks nothing; a shared
    context without the flag, fed the fleet that hears everything five times, is today's: every hearing is published."""
    fmt, filt, corr = N.FMT_CU8, "All Messages", "Conservative"
    srcs = fleet_sources(fmt)
    one = [srcs[1]]
    sched = schedule(one, fmt, seed=82, hi=30000)
    a = dedup_ctx(filt, corr, 1, STARTS[1:2], window=None)                # the default window
    b = ctx_of(SD | SH, filt, corr, 1, STARTS[1:2])
    ga, gb = run_dedup(a, fmt, one, sched, device=True), run(b, fmt, one, sched, device=True)
    for x, y in zip(ga, gb):
        assert x[1].tobytes() == y[1].tobytes() and x[3].tobytes() == y[3].tobytes() and np.array_equal(x[4], y[4])
        assert (x[5] == -1).all()
    assert a.stream_dedup_stats()[0] == 0 and sum(len(x[1]) for x in ga) > 240
    assert a.stream_planes()[0].tobytes() == b.stream_planes()[0].tobytes()
    a.close(), b.close()
    sched = schedule(srcs, fmt, seed=81, hi=40000)
    ctx = ctx_of(SD | SH, filt, corr, 5, STARTS)
    t = check(run(ctx, fmt, srcs, sched, device=True), plain_run(fmt, corr, srcs, sched, ("dedup", 81)), Expect(filt, corr, STARTS))
    assert t["records"] > 1200 and t["decoded"] > 400
    ctx.close()
