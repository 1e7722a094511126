"""The soft-decision CRC repair in a batch on the MI355X through the C ABI (ADSB_FLAG_FEC_SOFT_BATCH; include/adsb_hip.h: SOFT
REPAIR, IN A BATCH).  Items cut from tests/test_gpu_softfec.py's synthetic low-SNR stream go through adsb_process_batch* and,
as streams under several chunkings, through adsb_process_stream_batch*: records and adsb_batch_last_soft rows equal, item by item
and stream by stream, those of adsb_process_format + adsb_last_soft on an ADSB_FLAG_FEC_SOFT context and the plain restatement
tests/softfec_replay.py.  The CPU half is tests/test_softfec_batch.py, the kernel alone tests/test_gpu_softfec_batch_device.py."""
import numpy as np
import pytest

import softfec_cases as C
import softfec_replay as SR
import test_gpu_softfec as G
from gr_adsb_amd import _native as N

pytestmark = pytest.mark.gpu

FS, SPS, THR = G.FS, G.SPS, G.THR
S, SB, F = N.FLAG_FEC_SOFT, N.FLAG_FEC_SOFT_BATCH, N.FLAG_FEC_CONSERVATIVE
FMTS = {"mag2": N.FMT_MAG2, "sc16": N.FMT_SC16, "cu8": N.FMT_CU8}
EMPTY = np.zeros(0, dtype=N.BURST_DTYPE)
NOROWS = np.zeros(0, dtype=N.SOFT_DTYPE)


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


same = G.same


def cat(parts, empty=EMPTY):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else empty.copy()


# ---- adsb_process_batch* ------------------------------------------------------------------------------------------------
# eight items cut from the stream one behind the other: unequal lengths between 2^14 and 2^17, one empty, one at a stream
# offset of its own, one at a threshold of its own
LENS = (131072, 120000, 100001, 90002, 125000, 16384, 0, 110003)
ABS = (0, 0, 0, 1000000007, 0, 0, 0, 0)
THRS = (THR, THR, THR, THR, 0.008, THR, THR, THR)


def cut(fmt):
    """[(the item's samples in the format's layout, its float32 |IQ|^2)]"""
    data, x = G.stream(fmt)
    per = N.FMT_LAYOUT[fmt][1]
    out, lo = [], 0
    for n in LENS:
        out.append((np.ascontiguousarray(data[lo * per:(lo + n) * per]), x[lo:lo + n]))
        lo += n
    assert lo <= len(x)
    return out


def single_calls(fmt, flags, items):
    """item by item: (records, rows) of process_format + last_soft on an ADSB_FLAG_FEC_SOFT context with the same other flags, the
    replay over the item's raw records, and the records of a context with neither soft flag"""
    soft, raw, plain = G.make_ctx(S | flags, fmt), G.make_ctx(0, fmt), G.make_ctx(flags, fmt)
    out = []
    for (data, x), off, thr in zip(items, ABS, THRS):
        for c in (soft, raw, plain):
            c.set_threshold(thr)
        if len(x) == 0:
            out.append((EMPTY, NOROWS, EMPTY, NOROWS, EMPTY))
            continue
        recs = soft.process_format(fmt, data, abs_offset=off)
        rows = soft.last_soft()
        want, want_rows = SR.replay_records(raw.process_format(fmt, data, abs_offset=off), x, off, SPS, None, bool(flags & F))
        out.append((recs, rows, want, want_rows, plain.process_format(fmt, data, abs_offset=off)))
    for c in (soft, raw, plain):
        c.close()
    return out


@pytest.mark.parametrize("flags", [F, 0], ids=["with_conservative", "alone"])
@pytest.mark.parametrize("fmt_name", list(FMTS))
def test_process_batch_equals_the_single_calls_and_the_replay(native, fmt_name, flags):
    fmt = FMTS[fmt_name]
    items = cut(fmt)
    per_item = single_calls(fmt, flags, items)
    want = cat([p[2] for p in per_item])
    want_rows = cat([p[3] for p in per_item], NOROWS)
    first = np.concatenate([[0], np.cumsum([len(p[2]) for p in per_item])])
    print(fmt_name, "records", len(want), "soft repairs", int((want_rows["nflip"] > 0).sum()))
    assert (want_rows["nflip"] > 0).sum() >= 10                      # the replay itself repairs enough over the batch
    same(cat([p[0] for p in per_item]), want, "FEC_SOFT single calls equal the replay")
    same(cat([p[1] for p in per_item], NOROWS), want_rows, "FEC_SOFT single calls' rows equal the replay's")
    arrays = [d for d, _ in items]
    c = G.make_ctx(SB | flags, fmt)
    # host entry point
    recs, item_first = c.process_batch(fmt, arrays, list(THRS), list(ABS))
    assert c.last_batch_fallbacks == 0 and np.array_equal(item_first, first)
    same(recs, want, "process_batch")
    same(c.last_batch_soft(), want_rows, "process_batch rows")
    # device entry point
    ptrs = []
    try:
        for a in arrays:
            ptrs.append(c.device_alloc(max(a.nbytes, 16)))
            if a.nbytes:
                c.device_upload(ptrs[-1], a)
        recs, item_first = c.process_batch_device(fmt, ptrs, list(LENS), list(THRS), list(ABS))
        assert np.array_equal(item_first, first)
        same(recs, want, "process_batch_device")
        same(c.last_batch_soft(), want_rows, "process_batch_device rows")
    finally:
        for p in ptrs:
            c.device_free(p)
    # the ordinary entry point of the same context does what it does without the flag
    plain = G.make_ctx(flags, fmt)
    same(c.process_format(fmt, arrays[0]), plain.process_format(fmt, arrays[0]), "process_format on a FEC_SOFT_BATCH context")
    with pytest.raises(N.AdsbError):
        c.last_soft()
    # THE SAME CALL WITHOUT THE NEW FLAG: the unrepaired records
    recs0, item_first0 = plain.process_batch(fmt, arrays, list(THRS), list(ABS))
    assert np.array_equal(item_first0, first)
    same(recs0, cat([p[4] for p in per_item]), "without the flag")
    fixed = want_rows["nflip"] > 0
    assert (recs0["flags"][fixed] & (N.BURST_PARITY_OK | N.BURST_FEC_FIXED) == 0).all() and (recs["flags"][fixed] & N.BURST_PARITY_OK != 0).all()
    same(recs0[~fixed], want[~fixed], "records the soft rule left alone")
    with pytest.raises(N.AdsbError):
        plain.last_batch_soft()
    c.close(), plain.close()


def test_a_fallback_item_among_short_ones(native):
    """One cu8 item of 2^22 + 4096 samples (longer than ADSB_BATCH_ITEM_MAX) takes the ordinary pass inside the call: its records
    and rows are the single call's, spliced in at the item's place; adsb_last_result still names the call before."""
    fmt = N.FMT_CU8
    data, x = G.stream(fmt)
    big = np.ascontiguousarray(np.concatenate([data] * 4 + [data[:2 * 4096]]))
    assert len(big) // 2 == (1 << 22) + 4096 > N.BATCH_ITEM_MAX
    arrays = [np.ascontiguousarray(data[:2 * 20000]), big, np.ascontiguousarray(data[2 * 30000:2 * 60000])]
    soft = G.make_ctx(S | F, fmt)
    per = [(soft.process_format(fmt, a), soft.last_soft()) for a in arrays]
    assert (per[1][1]["nflip"] > 0).sum() >= 10
    c = G.make_ctx(SB | F, fmt)
    before = c.process_format(fmt, arrays[0])
    recs, first = c.process_batch(fmt, arrays)
    assert c.last_batch_fallbacks == 1 and list(first) == list(np.concatenate([[0], np.cumsum([len(p[0]) for p in per])]))
    same(recs, cat([p[0] for p in per]), "records")
    same(c.last_batch_soft(), cat([p[1] for p in per], NOROWS), "rows")
    same(c.last_result(), before, "adsb_last_result is left alone")
    # and the ordinary pass of the context has not kept the switch
    plain = G.make_ctx(F, fmt)
    same(c.process_format(fmt, arrays[2]), plain.process_format(fmt, arrays[2]), "process_format afterwards")


# ---- adsb_process_stream_batch* -------------------------------------------------------------------------------------------
NSTREAM = 1 << 17
SEAM = 60000                      # a chunk seam of the 30000-sample chunking
P_SEAM, P_LATE = SEAM - 130, 2 * 30000 + 30000 - 300      # a reply across that seam; one whose last sample arrives 60 samples before a seam


def hand_reply(x, p, rng, wrong):
    """a DF 17 reply written by hand into the float32 |IQ|^2 stream x at p: preamble, 112 bits at full scale over a quiet
    floor, and three wrong bits whose two samples are nearly equal (key 0.9) -> the transmitted frame"""
    x[p - 40:p + 300] = (rng.random(340, dtype=np.float32) * np.float32(0.0004)).astype(np.float32)
    for k in (0, 2, 7, 9):
        x[p + k] = 1.0
    f = C.frame(17, rng)
    bits = C.flipped(f, wrong)
    for i in range(112):
        s1 = p + 8 * SPS + i * SPS
        hi, lo = (np.float32(0.6), np.float32(0.54)) if i in wrong else (np.float32(1.0), x[s1])
        x[s1], x[s1 + 1] = (hi, lo) if bits[i] else (lo, hi)
    return f


def stream_source():
    x = G.stream(N.FMT_MAG2)[1][:NSTREAM].copy()
    rng = np.random.default_rng(99)
    # weak bits on both sides of the seam: bit i lies at p + 16 + 2 i, the seam at p + 130 = bit 57
    truth = {P_SEAM: hand_reply(x, P_SEAM, rng, [20, 56, 90]), P_LATE: hand_reply(x, P_LATE, rng, [9, 60, 100])}
    return x, truth


def drive(ctx, x, cuts, cap=None):
    """stream i pushes the chunks cuts[i] of x, one call per round for the streams that still have one, then END for all
    -> per stream: (records, rows, per call [(records, rows)])"""
    k = len(cuts)
    pos, nxt, got = [0] * k, [0] * k, [[] for _ in range(k)]
    while any(nxt[i] < len(cuts[i]) for i in range(k)):
        live = [i for i in range(k) if nxt[i] < len(cuts[i])]
        ns = [cuts[i][nxt[i]] for i in live]
        recs, first = ctx.process_stream_batch(N.FMT_MAG2, live, [x[pos[i]:pos[i] + n] for i, n in zip(live, ns)], cap=cap)
        rows = ctx.last_batch_soft()
        assert len(rows) == len(recs)
        for j, i in enumerate(live):
            got[i].append((recs[first[j]:first[j + 1]], rows[first[j]:first[j + 1]], pos[i] + ns[j]))
            pos[i] += ns[j]
            nxt[i] += 1
    recs, first = ctx.process_stream_batch(N.FMT_MAG2, list(range(k)), [x[:0]] * k, end=True)
    rows = ctx.last_batch_soft()
    for i in range(k):
        assert pos[i] == len(x)
        got[i].append((recs[first[i]:first[i + 1]], rows[first[i]:first[i + 1]], pos[i]))
    return [(cat([g[0] for g in gi]), cat([g[1] for g in gi], NOROWS), gi) for gi in got]


def fixed_cuts(n, step, head=()):
    out, left = list(head), n - sum(head)
    while left > 0:
        out.append(min(step, left))
        left -= out[-1]
    return out


@pytest.mark.parametrize("flags", [F, 0], ids=["with_conservative", "alone"])
def test_streams_under_three_chunkings_equal_one_call(native, flags):
    x, truth = stream_source()
    soft = G.make_ctx(S | flags)
    want = soft.process_format(N.FMT_MAG2, x)
    want_rows = soft.last_soft()
    # the two hand-placed replies are detected, and repaired to the transmitted frames, by the single call
    for p, f in truth.items():
        t = int(np.flatnonzero(want["offset"] == p)[0])
        assert want_rows[t]["nflip"] == 3 and SR.unpack(want["bits"][t]).tolist() == f.tolist(), p
    assert (want_rows["nflip"] > 0).sum() >= 2
    cuts = [fixed_cuts(NSTREAM, 1000), fixed_cuts(NSTREAM, 30000), fixed_cuts(NSTREAM, 4096, head=(7, 0, 1)), fixed_cuts(NSTREAM, 30000)]
    c = G.make_ctx(SB | flags)
    c.open_streams(4)
    got = drive(c, x, cuts)
    for i, (recs, rows, calls) in enumerate(got):
        same(recs, want, "stream %d records" % i)
        same(rows, want_rows, "stream %d rows" % i)
    assert all(c.stream_state(i)[2] == 0 for i in range(4))             # the condition under which equality is claimed
    # stream 1 (chunks of 30000): the reply across the seam at 60000 is delivered by the call that brought its second half, and
    # the reply that ends 60 samples before the seam at 90000 one call after its samples arrived
    calls = got[1][2]
    where = {p: [k for k, (r, _, _) in enumerate(calls) if p in r["offset"]] for p in truth}
    assert where[P_SEAM] == [2] and calls[1][2] == SEAM and calls[2][2] == 90000
    assert where[P_LATE] == [3] and P_LATE + 240 <= calls[2][2]
    # a call refused with -ENOSPC moves nothing: repeated with room it gives the same records and rows
    c2 = G.make_ctx(SB | flags)
    c2.open_streams(1)
    with pytest.raises(N.AdsbError) as e:
        c2.process_stream_batch(N.FMT_MAG2, [0], [x[:SEAM + 30000]], cap=3)
    assert e.value.code == -28 and c2.stream_state(0)[0] == 0
    again = drive(c2, x, [[SEAM + 30000] + fixed_cuts(NSTREAM - SEAM - 30000, 30000)])[0]
    same(again[0], want, "after -ENOSPC: records")
    same(again[1], want_rows, "after -ENOSPC: rows")
    # the same pushes without the new flag: the replies stay parity failures
    plain = G.make_ctx(flags)
    plain.open_streams(1)
    recs0 = cat([plain.process_stream_batch(N.FMT_MAG2, [0], [x])[0], plain.process_stream_batch(N.FMT_MAG2, [0], [x[:0]], end=True)[0]])
    assert np.array_equal(recs0["offset"], want["offset"])
    for p in truth:
        assert recs0["flags"][recs0["offset"] == p][0] & (N.BURST_PARITY_OK | N.BURST_FEC_FIXED) == 0


# ---- with ADSB_FLAG_STREAM_DECODE: every stream's decoder sees the repaired replies -----------------------------------------
def test_stream_decoders_equal_the_one_receiver_context(native):
    """The stream-decode invariant with the flag on both sides: per stream, the records and decoded rows over all calls are those
    of an AIRCRAFT_TABLE | DECODE | FEC_SOFT context over the whole stream."""
    import decode_streams as DS
    T, DEC, SD = N.FLAG_AIRCRAFT_TABLE, N.FLAG_DECODE, N.FLAG_STREAM_DECODE
    x = G.stream(N.FMT_MAG2)[1]
    starts = [G.START, G.START + 0.37]
    ref = G.make_ctx(S | F | T | DEC)
    c = G.make_ctx(SB | F | SD)
    c.open_streams(2)
    c.set_streams_decoder("All Messages")
    for s, t in enumerate(starts):
        c.set_stream_start(s, t)
    cuts = [fixed_cuts(len(x), 100000), fixed_cuts(len(x), 37003)]
    pos, got = [0, 0], [[], []]
    k = 0
    while any(pos[i] < len(x) for i in range(2)):
        live = [i for i in range(2) if pos[i] < len(x)]
        ns = [cuts[i][k] if k < len(cuts[i]) else 0 for i in live]
        recs, first = c.process_stream_batch(N.FMT_MAG2, live, [x[pos[i]:pos[i] + n] for i, n in zip(live, ns)])
        dec, rows = c.last_stream_decoded(), c.last_batch_soft()
        for j, i in enumerate(live):
            got[i].append((recs[first[j]:first[j + 1]], dec[first[j]:first[j + 1]], rows[first[j]:first[j + 1]]))
            pos[i] += ns[j]
        k += 1
    recs, first = c.process_stream_batch(N.FMT_MAG2, [0, 1], [x[:0]] * 2, end=True)
    dec, rows = c.last_stream_decoded(), c.last_batch_soft()
    for i in range(2):
        got[i].append((recs[first[i]:first[i + 1]], dec[first[i]:first[i + 1]], rows[first[i]:first[i + 1]]))
    for i in range(2):
        assert c.stream_state(i)[2] == 0
        ref.reset()
        ref.set_decoder("All Messages", starts[i])
        want = ref.process_format(N.FMT_MAG2, x)
        want_dec, want_rows = ref.last_decoded(), ref.last_soft()
        same(cat([g[0] for g in got[i]]), want, "stream %d records" % i)
        same(cat([g[2] for g in got[i]], NOROWS), want_rows, "stream %d soft rows" % i)
        DS.assert_rows_equal(cat([g[1] for g in got[i]], np.zeros(0, dtype=N.DECODED_DTYPE)), want_dec)
        soft = want_rows["nflip"] > 0
        assert soft.sum() >= 10 and (want_dec["port"][soft] != N.DEC_NONE).any()


# ---- end to end: a weak hearing joins its reply's group ---------------------------------------------------------------------
WRONG_BITS = (17, 52, 95)                     # three scattered, non-adjacent bits


def weak_source(TM):
    """receiver 1's source: the common one, where every twentieth extended squitter has three wrong bits whose two chips are
    drawn so that the wrong one wins with key about 0.6 (|IQ|^2 1.0 against 0.6)"""
    z = TM.iq_of(TM.replies(), 5).copy()
    rows = np.unpackbits(TM.replies(), axis=1)[:, :112]
    for k in TM.FLIPPED:
        s = 200 * SPS + TM.SLOT * k
        for i in WRONG_BITS:
            right = s + 8 * SPS + i * SPS + (0 if rows[k][i] else 1)
            wrong = s + 8 * SPS + i * SPS + (1 if rows[k][i] else 0)
            z[right] += np.float32(np.sqrt(0.6) - 1.0)
            z[wrong] += np.float32(1.0)
    return z


def push_rows(ctx, srcs, cuts):
    """test_gpu_mlat.push's host calls, keeping every delivered record's decoded row -> [(stream, record, row, call)]"""
    got = []
    n_rx = len(srcs)
    edges = [[0] + list(c) + [len(srcs[s])] for s, c in enumerate(cuts)]
    for k in range(len(edges[0])):
        end = k == len(edges[0]) - 1
        ids = list(range(n_rx)) if end else [int(i) for i in np.random.default_rng(k).permutation(n_rx)]
        parts = [srcs[i][:0] if end else srcs[i][edges[i][k]:edges[i][k + 1]] for i in ids]
        r, first = ctx.process_stream_batch(N.FMT_FC32, ids, parts, end=end)
        d = ctx.last_stream_decoded()
        got += [(ids[j], r[t], d[t], k) for j in range(len(ids)) for t in range(first[j], first[j + 1])]
    return got


def test_a_weak_hearing_joins_its_group_and_the_fix_has_six_receivers(native):
    import test_gpu_mlat as TM
    from oracle import adsb_oracle as O
    from test_mlat import compare
    z1 = weak_source(TM)
    truth = np.unpackbits(TM.replies(), axis=1)[:, :112]
    # on the CPU: the wrong bits are the reply's weakest under the noise, the Conservative table does not explain them, and the
    # replay repairs every one of the replies to the transmitted frame
    x1 = O.mag2(z1)
    o = O.run_stream(x1, TM.FS, TM.THR)
    for k in TM.FLIPPED:
        s = 200 * SPS + TM.SLOT * k
        t = int(np.flatnonzero(o["pdu_offsets"] == s)[0])
        bits = o["pdu_bits"][t]
        assert sorted(np.flatnonzero(bits != truth[k])) == list(WRONG_BITS) and SR.conservative(bits, 112) is None
        key = SR.sample_keys(x1, s, SPS)
        assert sorted(SR.candidates(key, 112, 3, 0.0)) == list(WRONG_BITS) and all(0.5 < key[i] < 0.7 for i in WRONG_BITS)
        b2, fixed, row = SR.soft_rule(bits, key)
        assert fixed and b2.tolist() == truth[k].tolist()
    assert TM.STARTS[1] > min(TM.STARTS)                       # receiver 1 is not the first to hear a reply
    srcs = [TM.sources()[0], z1] + [TM.sources()[0]] * (TM.N_RX - 2)
    weak = set(TM.replies()[k].tobytes() for k in TM.FLIPPED)
    for flag, n_heard in ((SB, TM.N_RX), (0, TM.N_RX - 1)):
        ctx = TM.mlat_ctx(extra=flag)
        got = push_rows(ctx, srcs, TM.CUTS_THREE)
        fixes, ms, mt = ctx.stream_mlat()
        delivered = [(s, r) for s, r, _, _ in got]
        lst, exp, ems, emt, ld = TM.oracle(delivered, TM.STARTS, TM.RX)
        compare("soft" if flag else "plain", fixes, ms, mt, exp, ems, emt, truth=TM.P, exp_ld=ld, converge=bool(flag))
        of_weak = np.array([f["bits"].tobytes() in weak for f in fixes])
        assert of_weak.sum() == len(TM.FLIPPED) and (fixes["n_heard"][of_weak] == n_heard).all() and (fixes["n_heard"][~of_weak] == TM.N_RX).all()
        at = set(200 * SPS + TM.SLOT * k for k in TM.FLIPPED)
        mine = [(r, d, k) for s, r, d, k in got if s == 1 and int(r["offset"]) in at]
        assert len(mine) == len(TM.FLIPPED)
        dups = 0
        for r, d, k in mine:
            # the reply's first hearing in publication order (delivered call, then arrival time) is published, the others are
            # duplicates: receiver 4 hears every reply before receiver 1, which is published only where its chunking delivered
            # the reply a call earlier
            others = [(k2, TM.STARTS[s2]) for s2, r2, _, k2 in got if s2 != 1 and r2["offset"] == r["offset"]]
            assert len(others) == TM.N_RX - 1
            if flag:
                assert r["bits"].tobytes() in weak and int(r["flags"]) & N.BURST_FEC_FIXED
                assert (d["port"] == N.DEC_DUPLICATE) == (min(others) < (k, TM.STARTS[1]))
                dups += int(d["port"] == N.DEC_DUPLICATE)
            else:                                                # a published parity failure, alone with its payload
                assert r["bits"].tobytes() not in weak and not int(r["flags"]) & (N.BURST_PARITY_OK | N.BURST_FEC_FIXED)
                assert d["port"] != N.DEC_DUPLICATE
        assert dups >= (len(mine) - 2 if flag else 0)
        ctx.close()
