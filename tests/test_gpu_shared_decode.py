"""ADSB_FLAG_STREAM_DECODE_SHARED on the MI355X, through the C ABI: one decoder behind all receiver streams (adsb_shared.hip's
time order around the k_fleet_* decode step).  Every call's verdict flags equal tests/aircraft_replay.py and its rows equal
tests/decode_replay.py over the call's records in the order (timestamp, list position), calls concatenated; the records
themselves are those of a context without any decoder.  Cross-receiver positions, the plane calls, a refused call, a fallback
item, the refusals, and a per-stream context beside it, unchanged.  The CPU half (emulator, the reference's golden) is
tests/test_shared_decode.py."""
import numpy as np
import pytest

import aircraft_replay as A
import decode_replay as D
import decode_streams as S
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from gr_adsb_amd import modulator as M
from test_gpu_decode import THR, stream
from test_gpu_stream_decode import CU8_SCALE, _code, cat, sparse_mag2, whole
from test_stream_decode import ISO_ADDR

pytestmark = pytest.mark.gpu

F, SD, SH, AGES = N.FLAG_FEC_CONSERVATIVE, N.FLAG_STREAM_DECODE, N.FLAG_STREAM_DECODE_SHARED, N.FLAG_PLANE_AGES
AP_BITS = N.BURST_AP_KNOWN | N.BURST_AP_FEC
ENOSPC, EINVAL = 28, 22
FS = 2e6
STARTS = [1760000000.625, 1760000000.995, 1760000000.125, -0.25]      # overlapping real times, and one stream that starts below zero


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


def ctx_of(flags, filt, corr, n_streams, starts):
    c = N.Context(FS, THR, flags=flags | (F if corr == "Conservative" else 0))
    c.set_format_scale(N.FMT_CU8, CU8_SCALE)
    c.open_streams(n_streams)
    if flags & SD:
        c.set_streams_decoder(filt)
        for s, t in enumerate(starts):
            c.set_stream_start(s, t)
    return c


def shared_ctx(filt, corr, n_streams, starts, extra=0):
    return ctx_of(SD | SH | extra, filt, corr, n_streams, starts)


class Expect:
    """ONE decoder behind the fleet, in plain Python: every call's records in the order (ts, t), calls concatenated."""

    def __init__(self, filt, corr, starts):
        self.dec, self.known, self.starts = D.Decoder(filt, corr), set(), starts

    def call(self, recs, first, ids):
        """recs: the call's records without verdict flags -> (records with them, rows, order)"""
        n = len(recs)
        stream_of = np.repeat(np.asarray(ids, np.int64), np.diff(np.asarray(first[:len(ids) + 1], np.int64)))
        assert len(stream_of) == n
        ts = [self.starts[int(s)] + int(o) / FS for s, o in zip(stream_of, recs["offset"])]
        order = sorted(range(n), key=lambda t: (ts[t], t))
        pub = [t for t in order if recs["flags"][t] & N.BURST_DEMOD]
        want = recs.copy()
        rows = np.zeros(n, dtype=N.DECODED_DTYPE)
        rows["icao"] = -1                                   # a record without a PDU: tests/test_gpu_stream_decode.py expect_rows
        rows["bits"] = recs["bits"]
        rows["df"] = recs["bits"][:, 0] >> 3
        rows["latitude"] = rows["longitude"] = np.nan
        if pub:
            want["flags"][pub] |= A.replay(recs["bits"][pub], self.dec.fec, self.known)[0]
            rows[pub] = S.to_rows([self.dec.row(recs["bits"][t], ts[t]) for t in pub])
        return want, rows, np.array(order, np.int32)


def schedule(srcs, fmt, seed, hi=200000):
    """[(ids, [lo, hi) per id, end)]: random chunks to random subsets in random item order until every source is used up, an
    item without samples in the second call, then END items for all."""
    per = N.FMT_LAYOUT[fmt][1]
    rng = np.random.default_rng(seed)
    k = len(srcs)
    total = [len(s) // per for s in srcs]
    pos, out = [0] * k, []
    while any(pos[i] < total[i] for i in range(k)):
        live = [int(i) for i in rng.permutation(k) if pos[i] < total[i] and rng.random() < 0.7]
        if not live:
            continue
        ns = [min(int(rng.integers(0, hi + 1)), total[i] - pos[i]) for i in live]
        if len(out) == 1:
            ns[0] = 0
        out.append((live, [(pos[i], pos[i] + n) for i, n in zip(live, ns)], False))
        for i, n in zip(live, ns):
            pos[i] += n
    out.append(([int(i) for i in rng.permutation(k)], [(total[i], total[i]) for i in range(k)], True))
    assert len(out) >= 5
    return out


def run(ctx, fmt, srcs, sched, device=False, decode=True, shared=True):
    """The schedule through one context -> [(ids, records, item_first, rows, order)]"""
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
        out.append((ids, r, first.copy(), ctx.last_stream_decoded() if decode else None, ctx.last_stream_order() if shared else None))
    for b in bases:
        ctx.device_free(b)
    return out


def check(got, plain, exp):
    """Every call of a shared context against the records of a context without a decoder and the plain-Python expectation"""
    tally = dict(records=0, known=0, fec=0, decoded=0)
    for (ids, r, first, rows, order), (_, pr, pfirst, _, _) in zip(got, plain):
        assert list(first) == list(pfirst) and len(r) == len(pr) == len(rows) == len(order) == first[len(ids)]
        assert not (pr["flags"] & AP_BITS).any()
        want, wrows, worder = exp.call(pr, first, ids)
        assert np.array_equal(order, worder)
        assert r.tobytes() == want.tobytes()
        if len(r):
            S.assert_rows_equal(rows, wrows)
        tally["records"] += len(r)
        tally["known"] += int((r["flags"] & N.BURST_AP_KNOWN != 0).sum())
        tally["fec"] += int((r["flags"] & N.BURST_AP_FEC != 0).sum())
        tally["decoded"] += int((rows["port"] == N.DEC_DECODED).sum())
    return tally


_src = {}


def fleet_sources(fmt):
    """Four receivers that hear the same 40 aircraft: decode_streams.mixed traffic, about 1200 bursts and 0.5 M samples each"""
    if fmt not in _src:
        out = []
        for s in range(4):
            b14, _ = S.mixed(np.random.default_rng(500 + s), n=1200, addresses=ISO_ADDR, t0=0.0, dt=(0.002, 0.05))
            iq, _ = stream(b14, FS)
            out.append(iq if fmt == N.FMT_FC32 else M.quantize_iq8(iq, offset_binary=True))
        _src[fmt] = out
    return _src[fmt]


_plain = {}


def plain_run(fmt, corr, srcs, sched, key):
    """The schedule's records from a context without any decoder (cached: they do not depend on msg_filter)"""
    k = (fmt, corr, key)
    if k not in _plain:
        c = ctx_of(0, None, corr, len(srcs), [])
        _plain[k] = run(c, fmt, srcs, sched, decode=False, shared=False)
        c.close()
    return _plain[k]


# ---- 1. flags, rows and order equal one decoder fed in time order ---------------------------------------------------------
@pytest.mark.parametrize("filt", ["All Messages", "Extended Squitter Only"])
@pytest.mark.parametrize("corr", ["None", "Conservative"])
@pytest.mark.parametrize("fmt_name", ["fc32", "cu8"])
def test_flags_rows_and_order_equal_one_decoder_in_time_order(native, fmt_name, corr, filt):
    """Random chunks to random subsets in random item order, an n == 0 item and END items; fc32 through the host entry point,
    cu8 through the device one."""
    fmt = {"fc32": N.FMT_FC32, "cu8": N.FMT_CU8}[fmt_name]
    srcs = fleet_sources(fmt)
    sched = schedule(srcs, fmt, seed=71)
    ctx = shared_ctx(filt, corr, 4, STARTS)
    got = run(ctx, fmt, srcs, sched, device=(fmt == N.FMT_CU8))
    assert all(ctx.stream_state(s)[2] == 0 for s in range(4))
    t = check(got, plain_run(fmt, corr, srcs, sched, 71), Expect(filt, corr, STARTS))
    print(t)
    assert t["records"] > 4500 and t["decoded"] > 1500
    if filt == "All Messages":
        assert t["known"] > 400
    planes, cap, grows = ctx.stream_decoder_stats()
    assert planes == 40 and grows == 0                     # one plane per aircraft, whoever heard it
    rows, first = ctx.stream_planes()
    assert list(first) == [0, 40, 40, 40, 40] and sorted(rows["icao"].tolist()) == sorted(ISO_ADDR)
    ctx.close()


def test_one_call_beyond_a_sort_tile(native):
    """All four streams whole in one call: more than 4096 records, so the pair sort crosses a tile; then the END items."""
    fmt, filt, corr = N.FMT_CU8, "All Messages", "Conservative"
    srcs = fleet_sources(fmt)
    per = N.FMT_LAYOUT[fmt][1]
    total = [len(s) // per for s in srcs]
    sched = [([2, 0, 3, 1], [(0, total[i]) for i in (2, 0, 3, 1)], False), ([0, 1, 2, 3], [(total[i], total[i]) for i in range(4)], True)]
    ctx = shared_ctx(filt, corr, 4, STARTS)
    got = run(ctx, fmt, srcs, sched, device=True)
    assert len(got[0][1]) > 4096
    t = check(got, plain_run(fmt, corr, srcs, sched, "whole"), Expect(filt, corr, STARTS))
    assert t["records"] > 4500 and t["known"] > 400 and ctx.stream_decoder_stats()[0] == 40
    ctx.close()


# ---- 2. what only a shared decoder can do ---------------------------------------------------------------------------------
PA, AB, AC, AD = 0x4B1A01, 0x3C65A2, 0xA0F003, 0x71BC04
LAT, LON = 47.1, 8.5


def df11(aa):
    f = np.zeros(112, np.uint8)
    f[:5], f[5:8], f[8:32] = S.ib(11, 5), S.ib(5, 3), S.ib(aa, 24)
    f[32:56] = S.ib(M.crc24(f[:32]), 24)
    return f


def position(aa, odd, lat, lon):
    la, lo = S.cpr_encode(lat, lon, odd)
    body = np.zeros(51, np.uint8)
    body[3:15], body[16], body[17:34], body[34:51] = S.ib(0xC38, 12), odd, S.ib(la, 17), S.ib(lo, 17)
    return S.es(aa, 11, body)


def ident(aa, code):
    body = np.zeros(51, np.uint8)
    for k in range(8):
        body[3 + 6 * k:9 + 6 * k] = S.ib(code, 6)
    return S.es(aa, 4, body)


def pair_sources():
    """Two receivers with equal starts whose bursts sit in the same slots, so that slot k of both is a bit-equal tie and the
    item order [1, 0] publishes stream 1's PDU first.  -> (sources, {case: (stream, slot)})"""
    if "pair" not in _src:
        rng = np.random.default_rng(77)
        s0 = [ident(0x100000 + k, 1 + k % 50) for k in range(24)]
        s1 = [ident(0x200000 + k, 2 + k % 50) for k in range(24)]
        where = {}
        s0[1] = df11(AB); s1[3] = S.ap(4, AB, rng); where["b"] = (1, 3)             # announced on 0 (later in the list), slot 1 < 3: known
        s1[8] = df11(AC); s0[7] = S.ap(20, AC, rng); where["c"] = (0, 7)            # announced on 1 (earlier in the list), slot 8 > 7: not
        s1[10] = S.ap(5, AD, rng); s0[10] = df11(AD); where["d"] = (1, 10)          # the same slot: stream 1's reply goes first: not
        for k, slot in enumerate((12, 14, 16, 18)):                                 # (a) even frames on 0, odd frames on 1
            (s1 if k % 2 else s0)[slot] = position(PA, k % 2, LAT + 0.001 * k, LON)
        srcs = [stream(np.packbits(np.array(s, np.uint8), axis=1), FS)[0] for s in (s0, s1)]
        _src["pair"] = srcs, where, stream(np.packbits(np.array(s0, np.uint8), axis=1), FS)[1]
    return _src["pair"]


def test_cases_across_receivers(native):
    """(a) an aircraft whose even frames one receiver hears and whose odd frames the other gets a position -- and none on a
    per-stream context fed the same data; (b) a reply to an address announced on the other stream earlier in time is known;
    (c) announced later in time, earlier in the list: not known; (d) a bit-equal tie goes to the item passed first."""
    srcs, where, slots = pair_sources()
    fmt, filt, corr = N.FMT_FC32, "All Messages", "None"
    starts = [1760000000.5, 1760000000.5]
    n = len(srcs[0])
    sched = [([1, 0], [(0, n), (0, n)], False), ([1, 0], [(n, n), (n, n)], True)]
    ctx = shared_ctx(filt, corr, 2, starts, extra=AGES)
    got = run(ctx, fmt, srcs, sched)
    check(got, plain_run(fmt, corr, srcs, sched, "pair"), Expect(filt, corr, starts))
    ids, r, first, rows, order = got[0]
    assert ids == [1, 0] and len(r) >= 48
    at = {}                                                # (stream, slot) -> list position: the item's record nearest the burst
    for item, s_ in enumerate(ids):
        off = r["offset"][first[item]:first[item + 1]].astype(np.int64)
        for k, b in enumerate(slots):
            j = int(np.argmin(np.abs(off - int(b))))
            assert abs(int(off[j]) - int(b)) < 64, (s_, k)
            at[(s_, k)] = int(first[item]) + j
    known = {c: bool(r["flags"][at[w]] & N.BURST_AP_KNOWN) for c, w in where.items()}
    assert known == {"b": True, "c": False, "d": False}
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    for k in range(len(slots)):                            # every slot a bit-equal tie: the item passed first goes first
        assert r["offset"][at[(1, k)]] == r["offset"][at[(0, k)]] and rank[at[(1, k)]] + 1 == rank[at[(0, k)]], k
    # (a): the shared decoder's plane has a position; the plane calls report it as stream 0's
    prow, first_p = ctx.stream_planes()
    assert first_p[0] == 0 and list(first_p[1:]) == [len(prow)] * 2
    pa = prow[prow["icao"] == PA]
    assert len(pa) == 1 and abs(float(pa["latitude"][0]) - (LAT + 0.003)) < 0.001 and abs(float(pa["longitude"][0]) - LON) < 0.001
    assert ctx.stream_decoder_stats()[0] == len(prow)
    # ... as do the merged picture and the expiry
    mrows, info = ctx.merged_planes(None, None)
    assert (info["n_streams"] == 1).all() and all(np.array_equal(mrows[k], prow[k], equal_nan=(k == "latitude"))
                                                     for k in ("icao", "num_msgs", "callsign", "latitude"))
    assert ctx.expire_stream_planes(np.array([1 << 62, 0], np.int64)) == len(prow) and ctx.stream_decoder_stats()[0] == 0
    ctx.close()
    # a decoder per stream, the same data: no position in either table
    per = ctx_of(SD, filt, corr, 2, starts)
    run(per, fmt, srcs, sched, shared=False)
    prow2, first2 = per.stream_planes()
    both = prow2[prow2["icao"] == PA]
    assert len(both) == 2 and np.isnan(both["latitude"]).all() and first2[1] > 0 and first2[2] > first2[1]
    per.close()


def test_decoder_reset_stream_reset_and_the_front_end(native):
    """adsb_stream_reset leaves the shared decoder alone, adsb_streams_decoder_reset and adsb_reset make it fresh, an END item
    does not; frontend.Receivers(shared=True): .order beside .rows, and the plane calls without a stream index."""
    srcs, _, _ = pair_sources()
    fmt, filt, corr = N.FMT_FC32, "All Messages", "None"
    starts = [1760000000.5, 1760000000.5]
    fe = frontend.FrontEnd(FS, THR, flags=SD | SH | AGES)
    with pytest.raises(ValueError):
        fe.receivers(2, fmt=fmt)                           # a shared context wants shared=True
    rx = fe.receivers(2, fmt=fmt, starts=starts, msg_filter=filt, ages=True, shared=True)
    exp = Expect(filt, corr, starts)
    half = len(srcs[0]) // 2

    def push(parts, ids, finish=False):
        out = rx.finish(ids) if finish else rx.push(parts, ids=ids)
        recs, rows = cat(out, N.BURST_DTYPE), cat(rx.rows, N.DECODED_DTYPE)
        first = np.concatenate([[0], np.cumsum([len(o) for o in out])])
        plain = recs.copy()
        plain["flags"] &= ~np.uint16(AP_BITS)
        want, wrows, worder = exp.call(plain, first, ids)
        assert recs.tobytes() == want.tobytes() and np.array_equal(rx.order, worder)
        if len(recs):
            S.assert_rows_equal(rows, wrows)

    push([srcs[1][:half], srcs[0][:half]], [1, 0])
    n_planes = len(rx.planes())
    assert n_planes > 20 and fe.ctx.stream_decoder_stats()[0] == n_planes
    fe.ctx.reset_stream(1)                                 # framing only: the planes stay
    assert fe.ctx.stream_state(1)[0] == 0 and fe.ctx.stream_state(0)[0] > 0 and len(rx.planes()) == n_planes
    push([srcs[1][:half]], [1])                            # the same samples again: every address is known by now
    push(None, [0, 1], finish=True)                        # END items: the decoder stays
    assert len(rx.planes()) == n_planes
    rows, seen = rx.planes(seen=True)
    assert len(rows) == n_planes and (seen == int(starts[0])).all()
    assert np.array_equal(rx.merged()[0]["icao"], rows["icao"]) and len(rx.table(starts[0] + 1.0)) > 0
    fe.ctx.reset_streams_decoder()
    exp = Expect(filt, corr, starts)
    assert len(rx.planes()) == 0 and fe.ctx.stream_decoder_stats()[0] == 0
    push([srcs[0][:half], srcs[1][:half]], [0, 1])
    assert len(rx.planes()) == n_planes
    assert rx.expire(int(starts[0]) + 1) == n_planes and len(rx.planes()) == 0
    exp = Expect(filt, corr, starts)                       # (every announced address had a plane: nothing is known any more)
    push([srcs[0][half:], srcs[1][half:]], [0, 1])
    fe.ctx.reset()                                         # every stream fresh, and the decoder
    assert fe.ctx.stream_decoder_stats()[0] == 0 and fe.ctx.stream_state(0)[0] == 0
    rx.close()
    fe.ctx.close()


# ---- 3. the guarantees of a stream-batch call -----------------------------------------------------------------------------
def test_a_refused_call_changes_nothing(native):
    fmt, filt, corr = N.FMT_FC32, "All Messages", "Conservative"
    srcs = fleet_sources(fmt)[:2]
    cuts_a, cuts_b = [150000, 90000], [330000, 250000]

    def go(ctx, refuse):
        out = [ctx.process_stream_batch(fmt, [1, 0], [srcs[i][:cuts_a[i]] for i in (1, 0)]) + (ctx.last_stream_decoded(), ctx.last_stream_order())]
        if refuse:
            before = [ctx.stream_state(i) for i in (0, 1)], ctx.stream_decoder_stats()
            assert before[1][0] > 30
            assert _code(ctx.process_stream_batch, fmt, [0, 1], [srcs[i][cuts_a[i]:cuts_b[i]] for i in (0, 1)], cap=3) == -ENOSPC
            assert ([ctx.stream_state(i) for i in (0, 1)], ctx.stream_decoder_stats()) == before
            assert len(ctx.last_stream_decoded()) == len(ctx.last_stream_order()) == len(out[0][0])
        out.append(ctx.process_stream_batch(fmt, [0, 1], [srcs[i][cuts_a[i]:cuts_b[i]] for i in (0, 1)]) + (ctx.last_stream_decoded(), ctx.last_stream_order()))
        out.append(ctx.process_stream_batch(fmt, [1, 0], [srcs[1][cuts_b[1]:], srcs[0][cuts_b[0]:]], end=True) + (ctx.last_stream_decoded(), ctx.last_stream_order()))
        return out, ctx.stream_decoder_stats()

    a, sa = go(shared_ctx(filt, corr, 2, STARTS[:2]), True)
    b, sb = go(shared_ctx(filt, corr, 2, STARTS[:2]), False)
    assert sa == sb and sa[0] == 40
    for (r1, f1, d1, o1), (r2, f2, d2, o2) in zip(a, b):
        assert r1.tobytes() == r2.tobytes() and list(f1) == list(f2) and d1.tobytes() == d2.tobytes() and np.array_equal(o1, o2)
    assert sum(len(x[0]) for x in a) > 2000


def test_a_fallback_item_is_decoded_with_the_rest(native):
    filt, corr, fmt = "All Messages", "Conservative", N.FMT_MAG2
    addr = ISO_ADDR[:12]
    b_long, _ = S.mixed(np.random.default_rng(61), n=400, addresses=addr)
    srcs = [sparse_mag2(b_long, N.BATCH_ITEM_MAX + 4096, 10000, 1)]
    for s in (1, 2):
        b, _ = S.mixed(np.random.default_rng(61 + s), n=200, addresses=addr)
        srcs.append(sparse_mag2(b, 200 * 400 + 1000, 400, 1 + s))
    sched = [([1, 0, 2], [(0, len(srcs[i])) for i in (1, 0, 2)], False), ([0, 1, 2], [(len(srcs[i]),) * 2 for i in range(3)], True)]
    ctx = shared_ctx(filt, corr, 3, STARTS[:3])
    out = []
    for ids, spans, end in sched:
        r, first = ctx.process_stream_batch(fmt, ids, [srcs[i][lo:hi] for i, (lo, hi) in zip(ids, spans)], end=end)
        if not end:
            assert ctx.last_batch_fallbacks == 1
        out.append((ids, r, first.copy(), ctx.last_stream_decoded(), ctx.last_stream_order()))
    t = check(out, plain_run(fmt, corr, srcs, sched, "fallback"), Expect(filt, corr, STARTS[:3]))
    assert t["records"] >= 780 and t["decoded"] > 150 and ctx.stream_decoder_stats()[0] == 12
    ctx.close()


def test_refusals(native):
    for flags in (SH, SH | N.FLAG_DECODE | N.FLAG_AIRCRAFT_TABLE, SH | AGES, SH | F):
        with pytest.raises(N.AdsbError) as e:
            N.Context(FS, THR, flags=flags)
        assert e.value.code == -EINVAL
    ctx = N.Context(FS, THR, flags=SD | SH | F | N.FLAG_LONG_AWARE_GATE | AGES)
    assert _code(ctx.last_stream_order) == -EINVAL and _code(ctx.reset_streams_decoder) == -EINVAL      # no streams yet
    ctx.open_streams(2)
    assert len(ctx.last_stream_order()) == 0
    ctx.reset_streams_decoder()
    r, first = ctx.process_stream_batch(N.FMT_FC32, [], [])
    assert len(r) == 0 and len(ctx.last_stream_order()) == 0
    ctx.close_streams()
    assert _code(ctx.last_stream_order) == -EINVAL
    ctx.close()
    per = N.Context(FS, THR, flags=SD)
    per.open_streams(2)
    assert _code(per.last_stream_order) == -EINVAL and _code(per.reset_streams_decoder) == -EINVAL
    per.close()
    plain = N.Context(FS, THR)
    assert _code(plain.last_stream_order) == -EINVAL and _code(plain.reset_streams_decoder) == -EINVAL
    plain.close()


# ---- 4. a per-stream context beside it ------------------------------------------------------------------------------------
def test_a_per_stream_context_is_untouched(native):
    """ADSB_FLAG_STREAM_DECODE without the shared flag, the same inputs and schedule: per stream the bytes of today -- those of a
    one-receiver context over the whole stream (tests/test_gpu_stream_decode.py whole())."""
    fmt, filt, corr = N.FMT_CU8, "All Messages", "Conservative"
    srcs = fleet_sources(fmt)[:3]
    sched = schedule(srcs, fmt, seed=72)
    ctx = ctx_of(SD, filt, corr, 3, STARTS[:3])
    got = run(ctx, fmt, srcs, sched, device=True, shared=False)
    for s in range(3):
        recs = cat([r[first[ids.index(s)]:first[ids.index(s) + 1]] for ids, r, first, _, _ in got if s in ids], N.BURST_DTYPE)
        rows = cat([d[first[ids.index(s)]:first[ids.index(s) + 1]] for ids, _, first, d, _ in got if s in ids], N.DECODED_DTYPE)
        want_recs, want_rows = whole(filt, corr, fmt, srcs[s], STARTS[s])
        assert recs.tobytes() == want_recs.tobytes() and rows.tobytes() == want_rows.tobytes() and len(recs) > 1000
    assert ctx.stream_decoder_stats()[0] == 120
    ctx.close()
