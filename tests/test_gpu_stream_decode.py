"""ADSB_FLAG_STREAM_DECODE on the MI355X: one decoder behind every receiver stream (k_fleet_* behind adsb_process_stream_batch*).
Per stream, the concatenated records and rows are byte-identical to what an ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE context
writes for one adsb_process_format call over the whole stream, and the rows to the plain-Python replay (tests/decode_replay.py)
of the published records; a refused call, a fallback item, growth of the store from its minimum, resets, the refusals, and a
context without the flag.  The CPU half (emulator) is tests/test_stream_decode.py."""
import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
import helpers
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from gr_adsb_amd import modulator as M
from test_gpu_decode import THR, stream
from test_stream_decode import ISO_ADDR

pytestmark = pytest.mark.gpu

T, F, DEC, SD = N.FLAG_AIRCRAFT_TABLE, N.FLAG_FEC_CONSERVATIVE, N.FLAG_DECODE, N.FLAG_STREAM_DECODE
ENOSPC, EINVAL = 28, 22
FS = 2e6
CU8_SCALE = 2.0 ** -6            # a power of two: k_detect's exact uint8 conversion
STARTS = [1760000000.625 + 0.37 * s for s in range(3)]    # whole-second boundaries inside each stream, different between streams


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


def _code(fn, *a, **k):
    with pytest.raises(N.AdsbError) as e:
        fn(*a, **k)
    return e.value.code


def fleet_ctx(filt, corr, n_streams, starts=None, extra=0):
    c = N.Context(FS, THR, flags=SD | (F if corr == "Conservative" else 0) | extra)
    c.set_format_scale(N.FMT_CU8, CU8_SCALE)
    c.open_streams(n_streams)
    c.set_streams_decoder(filt)
    for s, t in enumerate(starts or []):
        c.set_stream_start(s, t)
    return c


_ref = {}


def one_receiver(filt, corr):
    """ONE ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE context per configuration (1.5 GiB each), reset between streams"""
    key = (filt, corr)
    if key not in _ref:
        c = N.Context(FS, THR, flags=T | DEC | (F if corr == "Conservative" else 0))
        c.set_format_scale(N.FMT_CU8, CU8_SCALE)
        _ref[key] = c
    return _ref[key]


def whole(filt, corr, fmt, data, start):
    c = one_receiver(filt, corr)
    c.reset()
    c.set_decoder(filt, start)
    recs = c.process_format(fmt, data)
    return recs, c.last_decoded()


def expect_rows(recs, rep, start):
    """The rows of one stream's records: the replay for the records with BURST_DEMOD at start + offset / fs, a fixed row
    for the others (tests/test_gpu_decode.py expect_rows, with the stream's own start)."""
    out = np.zeros(len(recs), dtype=N.DECODED_DTYPE)
    dem = np.flatnonzero((recs["flags"] & N.BURST_DEMOD) != 0)
    out[dem] = S.to_rows(rep.rows(recs["bits"][dem], [start + int(o) / FS for o in recs["offset"][dem]]))
    rest = np.setdiff1d(np.arange(len(recs)), dem)
    out["icao"][rest] = -1
    out["bits"][rest] = recs["bits"][rest]
    out["df"][rest] = recs["bits"][rest, 0] >> 3
    out["latitude"][rest] = out["longitude"][rest] = np.nan
    return out


_replayed = {}


def replay_rows(recs, filt, corr, start):
    key = (recs.tobytes(), filt, corr, start)
    if key not in _replayed:
        _replayed[key] = expect_rows(recs, D.Decoder(filt, corr), start)
    return _replayed[key]


def rows_equal(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    if len(got):
        S.assert_rows_equal(got, exp)


def cat(parts, dtype):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)


def push_random(ctx, fmt, srcs, seed, hi=200000, device=False):
    """Random chunks of 0..hi samples to random subsets of the streams until every source is used up, then END items for all.
    -> per stream the concatenated records and rows"""
    per, bps = N.FMT_LAYOUT[fmt][1], N.FMT_BYTES[fmt]
    rng = np.random.default_rng(seed)
    k = len(srcs)
    pos, recs, rows = [0] * k, [[] for _ in range(k)], [[] for _ in range(k)]
    total = [len(s) // per for s in srcs]
    bases = []
    if device:
        for s in srcs:
            b = ctx.device_alloc(max(s.nbytes, 16))
            ctx.device_upload(b, np.ascontiguousarray(s))
            bases.append(b)
    rounds = 0
    while any(pos[i] < total[i] for i in range(k)):
        live = [i for i in range(k) if pos[i] < total[i] and rng.random() < 0.7]
        if not live:
            continue
        ns = [min(int(rng.integers(0, hi + 1)), total[i] - pos[i]) for i in live]
        if rounds == 1:
            ns[0] = 0                                   # an item without samples
        if device:
            r, first = ctx.process_stream_batch_device(fmt, live, [bases[i] + pos[i] * bps for i in live], ns)
        else:
            r, first = ctx.process_stream_batch(fmt, live, [srcs[i][pos[i] * per:(pos[i] + n) * per] for i, n in zip(live, ns)])
        d = ctx.last_stream_decoded()
        assert len(d) == len(r) == first[len(live)]
        for j, i in enumerate(live):
            recs[i].append(r[first[j]:first[j + 1]])
            rows[i].append(d[first[j]:first[j + 1]])
            pos[i] += ns[j]
        rounds += 1
    dt = N.FMT_LAYOUT[fmt][0]
    r, first = ctx.process_stream_batch(fmt, list(range(k)), [np.zeros(0, dtype=dt)] * k, end=True)
    d = ctx.last_stream_decoded()
    for i in range(k):
        recs[i].append(r[first[i]:first[i + 1]])
        rows[i].append(d[first[i]:first[i + 1]])
    for b in bases:
        ctx.device_free(b)
    assert rounds >= 4
    return [cat(x, N.BURST_DTYPE) for x in recs], [cat(x, N.DECODED_DTYPE) for x in rows]


_iso = {}


def iso_sources(fmt):
    """The isolation traffic of tests/test_stream_decode.py, one burst per 200 us over AWGN at -40 dB: about 0.5 M samples a stream"""
    if fmt not in _iso:
        out = []
        for s in range(3):
            b14, _ = S.mixed(np.random.default_rng(100 + s), n=1200, addresses=ISO_ADDR, t0=1760000000.5 + 0.37 * s, dt=(0.002, 0.05))
            iq, _ = stream(b14, FS)
            out.append(iq if fmt == N.FMT_FC32 else M.quantize_iq8(iq, offset_binary=True))
        _iso[fmt] = out
    return _iso[fmt]


def check_streams(ctx, recs, rows, srcs, fmt, filt, corr, starts, min_decoded=500):
    for s in range(len(srcs)):
        assert ctx.stream_state(s)[2] == 0                                  # nothing left out: equality is claimed
        want_recs, want_rows = whole(filt, corr, fmt, srcs[s], starts[s])
        assert recs[s].tobytes() == want_recs.tobytes(), ("records", s)
        rows_equal(rows[s], want_rows)
        exp = replay_rows(want_recs, filt, corr, starts[s])
        print("stream %d: %d records, %d PDUs, %d decoded rows in the replay" % (
            s, len(want_recs), int((want_recs["flags"] & N.BURST_DEMOD != 0).sum()), int((exp["port"] == N.DEC_DECODED).sum())))
        assert (exp["port"] == N.DEC_DECODED).sum() >= min_decoded           # from the replay alone
        rows_equal(rows[s], exp)


# ---- 1. rows equal the replay and the one-receiver context ----------------------------------------------------------------
@pytest.mark.parametrize("filt", ["All Messages", "Extended Squitter Only"])
@pytest.mark.parametrize("corr", ["None", "Conservative"])
@pytest.mark.parametrize("fmt_name", ["fc32", "cu8"])
def test_rows_equal_the_replay_and_the_one_receiver_context(native, fmt_name, corr, filt):
    fmt = {"fc32": N.FMT_FC32, "cu8": N.FMT_CU8}[fmt_name]
    srcs = iso_sources(fmt)
    ctx = fleet_ctx(filt, corr, 3, STARTS)
    recs, rows = push_random(ctx, fmt, srcs, seed=41)
    check_streams(ctx, recs, rows, srcs, fmt, filt, corr, STARTS)
    if filt == "All Messages":
        known = sum(int((r["flags"] & N.BURST_AP_KNOWN != 0).sum()) for r in recs)
        assert known > 300                                                  # the verdict flags are part of the match
    planes, cap, grows = ctx.stream_decoder_stats()
    assert planes == 120 and grows == 0 and cap == 1 << 16
    ctx.close()


def test_the_device_entry_point_and_the_front_end(native):
    filt, corr, fmt = "All Messages", "Conservative", N.FMT_CU8
    srcs = iso_sources(fmt)
    ctx = fleet_ctx(filt, corr, 3, STARTS)
    recs, rows = push_random(ctx, fmt, srcs, seed=42, device=True)
    check_streams(ctx, recs, rows, srcs, fmt, filt, corr, STARTS)
    ctx.close()
    # frontend.Receivers: .rows beside the returned record arrays
    fe = frontend.FrontEnd(FS, THR, flags=SD | F)
    fe.ctx.set_format_scale(fmt, CU8_SCALE)
    rx = fe.receivers(3, fmt=fmt, starts=STARTS, msg_filter=filt)
    got, drows = [[] for _ in range(3)], [[] for _ in range(3)]
    half = [len(s) // 4 * 2 for s in srcs]
    for parts, ids in (([srcs[0][:half[0]], srcs[2][:half[2]]], [0, 2]), ([srcs[1]], [1]), ([srcs[2][half[2]:], srcs[0][half[0]:]], [2, 0])):
        out = rx.push(parts, ids=ids)
        assert len(rx.rows) == len(out) == len(ids)
        for i, r, d in zip(ids, out, rx.rows):
            assert len(r) == len(d)
            got[i].append(r)
            drows[i].append(d)
    out = rx.finish()
    for i in range(3):
        got[i].append(out[i])
        drows[i].append(rx.rows[i])
    check_streams(fe.ctx, [cat(x, N.BURST_DTYPE) for x in got], [cat(x, N.DECODED_DTYPE) for x in drows], srcs, fmt, filt, corr, STARTS)
    # a row and its record's meta give the reference's published PDU
    r, d = cat(got[0], N.BURST_DTYPE), cat(drows[0], N.DECODED_DTYPE)
    i = int(np.flatnonzero(d["port"] == N.DEC_DECODED)[0])
    name, (meta, vec) = N.decoded_pdu(d[i], {"timestamp": STARTS[0] + int(r["offset"][i]) / FS, "snr": 30.0})
    assert name == "decoded" and meta["icao"] == "{:06x}".format(int(d["icao"][i])) and len(vec) == 112
    rx.close()
    fe.ctx.close()


# ---- 2. a refused call moves nothing ----------------------------------------------------------------------------------------
def test_a_refused_call_changes_no_decoder(native):
    filt, corr, fmt = "All Messages", "Conservative", N.FMT_FC32
    srcs = iso_sources(fmt)[:2]
    cutsA = [150000, 90000]
    cutsB = [330000, 250000]

    def run(ctx, refuse):
        out = []
        out.append(ctx.process_stream_batch(fmt, [0, 1], [srcs[i][:cutsA[i]] for i in (0, 1)]) + (ctx.last_stream_decoded(),))
        if refuse:
            before = [ctx.stream_state(i) for i in (0, 1)], ctx.stream_decoder_stats()
            assert before[1][0] > 50
            code = _code(ctx.process_stream_batch, fmt, [0, 1], [srcs[i][cutsA[i]:cutsB[i]] for i in (0, 1)], cap=3)
            assert code == -ENOSPC and ctx.last_stream_needed > 3
            assert ([ctx.stream_state(i) for i in (0, 1)], ctx.stream_decoder_stats()) == before
            assert len(ctx.last_stream_decoded()) == len(out[0][0])         # still the rows of the last DELIVERED call
        out.append(ctx.process_stream_batch(fmt, [0, 1], [srcs[i][cutsA[i]:cutsB[i]] for i in (0, 1)]) + (ctx.last_stream_decoded(),))
        out.append(ctx.process_stream_batch(fmt, [1, 0], [srcs[1][cutsB[1]:], srcs[0][cutsB[0]:]], end=True) + (ctx.last_stream_decoded(),))
        return out, ctx.stream_decoder_stats()

    a, sa = run(fleet_ctx(filt, corr, 2, STARTS[:2]), True)
    b, sb = run(fleet_ctx(filt, corr, 2, STARTS[:2]), False)
    assert sa == sb and sa[0] == 80
    for (r1, f1, d1), (r2, f2, d2) in zip(a, b):
        assert r1.tobytes() == r2.tobytes() and list(f1) == list(f2) and d1.tobytes() == d2.tobytes() and len(d1) == len(r1)
    assert sum(len(x[0]) for x in a) > 2000


# ---- 3. an item that takes the ordinary pass --------------------------------------------------------------------------------
def sparse_mag2(b14, n, step, seed):
    """float32 |IQ|^2 of n samples at 2 Msps: the rows one burst per `step` samples over AWGN at -40 dB"""
    rng = np.random.default_rng(seed)
    z = ((rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) *
         np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
    rows = np.unpackbits(b14, axis=1)[:, :112]
    for k, b in enumerate(rows):
        env = M.burst_waveform(b, 2)
        s = 400 + k * step
        z[s:s + len(env)] += env
    return M.mag2(z)


def test_a_fallback_item_is_decoded_like_the_others(native):
    filt, corr, fmt = "All Messages", "Conservative", N.FMT_MAG2
    n_long = N.BATCH_ITEM_MAX + 4096
    addr = ISO_ADDR[:12]
    b_long, _ = S.mixed(np.random.default_rng(61), n=400, addresses=addr)
    srcs = [sparse_mag2(b_long, n_long, 10000, 1)]
    for s in (1, 2):
        b, _ = S.mixed(np.random.default_rng(61 + s), n=200, addresses=addr)
        srcs.append(sparse_mag2(b, 200 * 400 + 1000, 400, 1 + s))
    ctx = fleet_ctx(filt, corr, 3, STARTS)
    r, first = ctx.process_stream_batch(fmt, [1, 0, 2], [srcs[1], srcs[0], srcs[2]])
    assert ctx.last_batch_fallbacks == 1
    d = ctx.last_stream_decoded()
    r2, first2 = ctx.process_stream_batch(fmt, [0, 1, 2], [srcs[0][:0]] * 3, end=True)
    d2 = ctx.last_stream_decoded()
    order = {1: 0, 0: 1, 2: 2}
    recs = [cat([r[first[order[s]]:first[order[s] + 1]], r2[first2[s]:first2[s + 1]]], N.BURST_DTYPE) for s in range(3)]
    rows = [cat([d[first[order[s]]:first[order[s] + 1]], d2[first2[s]:first2[s + 1]]], N.DECODED_DTYPE) for s in range(3)]
    check_streams(ctx, recs, rows, srcs, fmt, filt, corr, STARTS, min_decoded=80)
    ctx.close()


# ---- 4. growth on the device ------------------------------------------------------------------------------------------------
def test_the_store_grows_from_its_minimum_on_the_device(native):
    filt, corr, fmt = "All Messages", "Conservative", N.FMT_FC32
    b14, _ = S.mixed(np.random.default_rng(21), n=1500, addresses=[0x100000 + 7 * k for k in range(1500)])
    iq, _ = stream(b14, FS)
    ctx = fleet_ctx(filt, corr, 4, [0.0, 0.0, 0.0, STARTS[0]])
    ctx.stream_decoder_reserve(0)
    assert ctx.stream_decoder_stats() == (0, 256, 0)
    rep = D.Decoder(filt, corr)
    n = len(iq)
    bounds = [0, n // 7, n // 3, n // 2, (3 * n) // 4, n]
    recs, rows = [], []
    for k, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        r, _ = ctx.process_stream_batch(fmt, [3], [iq[lo:hi]], end=(hi == n))
        d = ctx.last_stream_decoded()
        rows_equal(d, expect_rows(r, rep, STARTS[0]))
        planes, cap, grows = ctx.stream_decoder_stats()
        assert planes == len(rep.planes) and cap & (cap - 1) == 0 and 2 * planes <= cap
        recs.append(r)
        rows.append(d)
    assert grows >= 3 and planes > 1000 and ctx.stream_state(3)[2] == 0
    assert _code(ctx.stream_decoder_reserve, 1 << 12) == -EINVAL             # live planes
    want_recs, want_rows = whole(filt, corr, fmt, iq, STARTS[0])
    assert cat(recs, N.BURST_DTYPE).tobytes() == want_recs.tobytes()
    rows_equal(cat(rows, N.DECODED_DTYPE), want_rows)
    ctx.reset_stream(3)
    assert ctx.stream_decoder_stats()[0] == 0
    ctx.stream_decoder_reserve(1000)                                         # nothing live: allowed again, rounded up
    assert ctx.stream_decoder_stats() == (0, 1024, grows)
    ctx.close()


# ---- 5. resets --------------------------------------------------------------------------------------------------------------
def test_resets_make_decoders_fresh_and_the_end_item_does_not(native):
    filt, corr, fmt = "All Messages", "None", N.FMT_FC32
    srcs = iso_sources(fmt)[:2]
    half = [len(s) // 2 for s in srcs]
    ctx = fleet_ctx(filt, corr, 2, STARTS[:2])
    reps = [D.Decoder(filt, corr) for _ in (0, 1)]

    def push(parts, end):
        r, first = ctx.process_stream_batch(fmt, [0, 1], parts, end=end)
        d = ctx.last_stream_decoded()
        for s in (0, 1):
            rows_equal(d[first[s]:first[s + 1]], expect_rows(r[first[s]:first[s + 1]], reps[s], STARTS[s]))
        return ctx.stream_decoder_stats()[0]

    # the END item: the streams are fresh afterwards, their decoders are not
    assert push([srcs[s][:half[s]] for s in (0, 1)], True) == 80
    assert [ctx.stream_state(s)[0] for s in (0, 1)] == [0, 0]
    assert push([srcs[s][half[s]:] for s in (0, 1)], False) == 80
    # adsb_stream_reset: stream 0's decoder starts over, stream 1's goes on
    ctx.reset_stream(0)
    reps[0] = D.Decoder(filt, corr)
    assert ctx.stream_decoder_stats()[0] == 40 and ctx.stream_state(1)[0] > 0
    assert _code(ctx.set_stream_start, 1, 5.0) == -EINVAL                    # stream 1 has consumed samples
    ctx.set_stream_start(0, STARTS[0])                                      # a fresh stream may
    r, first = ctx.process_stream_batch(fmt, [0, 1], [srcs[0][:half[0]], srcs[1][:0]], end=[True, True])
    d = ctx.last_stream_decoded()
    for s in (0, 1):
        rows_equal(d[first[s]:first[s + 1]], expect_rows(r[first[s]:first[s + 1]], reps[s], STARTS[s]))
    seen = d[:first[1]][(d[:first[1]]["present"] & N.DEC_HAS_PLANE) != 0]
    assert seen["num_msgs"][0] == 1 and ctx.stream_decoder_stats()[0] == 80
    # adsb_reset: every decoder
    ctx.reset()
    reps = [D.Decoder(filt, corr) for _ in (0, 1)]
    assert ctx.stream_decoder_stats()[0] == 0
    assert push([srcs[s][:half[s]] for s in (0, 1)], True) == 80
    ctx.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(native):
    for other in (DEC | T, T, N.FLAG_CONFIDENCE):
        with pytest.raises(N.AdsbError) as e:
            N.Context(FS, THR, flags=SD | other)
        assert e.value.code == -EINVAL
    iq = iso_sources(N.FMT_FC32)[0][:200000]
    b14 = np.zeros((3, 14), np.uint8)
    ctx = N.Context(FS, THR, flags=SD | F | N.FLAG_LONG_AWARE_GATE)
    assert _code(ctx.last_decoded) == -EINVAL
    assert _code(ctx.decode_pdus, b14, np.zeros(3)) == -EINVAL
    assert _code(ctx.set_decoder, "All Messages", 0.0) == -EINVAL
    assert _code(ctx.stream_decoder_stats) == -EINVAL and _code(ctx.stream_decoder_reserve, 512) == -EINVAL     # no streams yet
    assert _code(ctx.last_stream_decoded) == -EINVAL
    # the other entry points behave as on a context without the flag
    plain = N.Context(FS, THR, flags=F | N.FLAG_LONG_AWARE_GATE)
    want = plain.process_format(N.FMT_FC32, iq)
    assert len(want) > 400 and ctx.process_format(N.FMT_FC32, iq).tobytes() == want.tobytes()
    wb, wf = plain.process_batch(N.FMT_FC32, [iq[:90000], iq[90000:]])
    gb, gf = ctx.process_batch(N.FMT_FC32, [iq[:90000], iq[90000:]])
    assert gb.tobytes() == wb.tobytes() and list(gf) == list(wf)
    ctx.open_streams(2)
    assert _code(ctx.set_stream_start, 2, 0.0) == -EINVAL and _code(ctx.stream_decoder_reserve, (1 << 27) + 1) == -EINVAL
    ctx.process_stream_batch(N.FMT_FC32, [0], [iq])
    assert _code(ctx.set_stream_start, 0, 1.0) == -EINVAL                    # the stream has consumed samples
    ctx.close_streams()
    assert _code(ctx.stream_decoder_stats) == -EINVAL
    ctx.close()
    assert _code(plain.last_stream_decoded) == -EINVAL and _code(plain.set_streams_decoder) == -EINVAL
    assert _code(plain.set_stream_start, 0, 0.0) == -EINVAL and _code(plain.stream_decoder_reserve, 512) == -EINVAL
    plain.close()


# ---- 7. a context without the flag ------------------------------------------------------------------------------------------
def test_a_stream_batch_without_the_flag_is_untouched(native):
    from test_gpu_stream_batch import cuts_fixed, cuts_random, drive
    g = helpers.Golden("g2msps_df17")
    n = len(g.x)
    ctx = N.Context(g.fs, g.thr)
    ctx.open_streams(3)
    got, nfb = drive(ctx, N.FMT_FC32, [g.iq] * 3, [cuts_fixed(n, 4096), cuts_random(n, 3000, seed=11), cuts_random(n, 70000, seed=12)],
                     [g.thr] * 3)
    assert nfb == 0
    for r in got:
        helpers.assert_recs_match_golden(r, g, "single")
        assert not np.any(r["flags"] & (N.BURST_AP_KNOWN | N.BURST_AP_FEC))
    assert _code(ctx.stream_decoder_stats) == -EINVAL and _code(ctx.last_stream_decoded) == -EINVAL
    ctx.close()
