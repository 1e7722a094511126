"""The soft-decision CRC repair on the MI355X through the C ABI (ADSB_FLAG_FEC_SOFT; include/adsb_hip.h: SOFT REPAIR): a
synthetic low-SNR stream (seed 0, 2^20 samples at 2 Msps, replies at 6..14 dB) in all five input formats through the blocking,
submitted, host-fed and device-resident entry points and adsb_demod_work.  Records, flags and adsb_soft_fix rows equal the
plain restatement tests/softfec_replay.py applied to a flag-off context's records over the same converted samples; with the
aircraft table and the decode step the rows equal adsb_decode_pdus over the repaired PDUs.  The CPU half is tests/test_softfec.py."""
import numpy as np
import pytest

import softfec_replay as SR
from gr_adsb_amd import _native as N
from gr_adsb_amd import modulator as M
from oracle import adsb_oracle as O

pytestmark = pytest.mark.gpu

FS, SPS, THR, NSAMP = 2e6, 2, 0.004, 1 << 20
S, F, T, DEC = N.FLAG_FEC_SOFT, N.FLAG_FEC_CONSERVATIVE, N.FLAG_AIRCRAFT_TABLE, N.FLAG_DECODE
SCALE = {N.FMT_SC16: 2.0 / 32767.0, N.FMT_SC8: 2.0 / 127.0, N.FMT_CU8: 2.0 / 255.0}
FMTS = {"fc32": N.FMT_FC32, "mag2": N.FMT_MAG2, "sc16": N.FMT_SC16, "sc8": N.FMT_SC8, "cu8": N.FMT_CU8}
START = 1760000000.0


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


_cache = {}


def stream(fmt):
    """(the format's samples, the float32 |IQ|^2 the device makes of them)"""
    if "iq" not in _cache:
        _cache["iq"] = M.synth_iq(NSAMP, FS, 1500, 0, noise_power=1e-3, snr_db_range=(6, 14))
    if fmt not in _cache:
        iq = _cache["iq"]
        if fmt == N.FMT_FC32:
            _cache[fmt] = (iq, O.mag2(iq))
        elif fmt == N.FMT_MAG2:
            _cache[fmt] = (O.mag2(iq), O.mag2(iq))
        elif fmt == N.FMT_SC16:
            q = M.quantize_iq16(iq)
            _cache[fmt] = (q, O.mag2_iq16(q, SCALE[fmt]))
        else:
            q = M.quantize_iq8(iq, offset_binary=fmt == N.FMT_CU8)
            _cache[fmt] = (q, O.mag2_iq8(q, SCALE[fmt], offset_binary=fmt == N.FMT_CU8))
    return _cache[fmt]


def make_ctx(flags, fmt=None, rule=None):
    c = N.Context(FS, THR, flags=flags)
    if fmt in SCALE:
        c.set_format_scale(fmt, SCALE[fmt])
    if rule:
        c.set_soft_fec(**rule)
    return c


def raw_records(fmt):
    key = ("raw", fmt)
    if key not in _cache:
        data, x = stream(fmt)
        recs = make_ctx(0, fmt).process_format(fmt, data)
        o = O.run_stream(x, FS, THR)                              # a context without the flag: the records the oracle names
        assert np.array_equal(recs["offset"], o["tag_offsets"]) and (recs["flags"] & (SR.FEC_FIXED | SR.FEC_DF) == 0).all()
        dem = (recs["flags"] & N.BURST_DEMOD) != 0
        assert np.array_equal(np.unpackbits(recs["bits"][dem], axis=1)[:, :112], o["pdu_bits"])
        _cache[key] = recs
    return _cache[key]


def expected(fmt, with_conservative, rule=None, origin=0):
    key = ("want", fmt, with_conservative, tuple(sorted((rule or {}).items())))
    if key not in _cache:
        _cache[key] = SR.replay_records(raw_records(fmt), stream(fmt)[1], 0, SPS, rule, with_conservative)
    recs, rows = _cache[key]
    recs = recs.copy()
    recs["offset"] += origin
    return recs, rows


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("fmt_name", list(FMTS))
def test_records_and_rows_equal_the_replay(native, fmt_name):
    fmt = FMTS[fmt_name]
    data, x = stream(fmt)
    n = len(x)
    want, rows = expected(fmt, True)
    # the replay itself repairs enough on this input for the comparison to mean something
    soft = rows["nflip"] > 0
    cons = ((want["flags"] & N.BURST_FEC_FIXED) != 0) & ~soft
    print(fmt_name, "records", len(want), "soft repairs", int(soft.sum()), "Conservative repairs", int(cons.sum()))
    assert soft.sum() >= 10 and cons.sum() >= 1
    assert ((want["flags"][soft] & N.BURST_PARITY_OK) != 0).all()
    # blocking, host-fed: with the Conservative repair in front, and alone
    c = make_ctx(S | F, fmt)
    same(c.process_format(fmt, data), want, "process_format")
    same(c.last_soft(), rows, "rows")
    alone, alone_rows = expected(fmt, False)
    c1 = make_ctx(S, fmt)
    same(c1.process_format(fmt, data), alone, "soft alone")
    same(c1.last_soft(), alone_rows, "soft alone rows")
    assert (alone_rows["nflip"] > 0).sum() >= soft.sum()            # (alone it also takes what the table would have repaired)
    # the Conservative flag alone repairs exactly what it repairs beside the soft rule
    only_f = make_ctx(F, fmt).process_format(fmt, data)
    assert np.array_equal((only_f["flags"] & N.BURST_FEC_FIXED) != 0, cons)
    same(only_f[~soft], want[~soft], "records the soft rule left alone")
    # submitted, host-fed: two passes in flight, waited for newest first; timed contexts run the tail behind an event
    for extra in (0, N.FLAG_TIMING):
        c = make_ctx(S | F | extra, fmt)
        t1 = c.submit_format_host(fmt, data)
        t2 = c.submit_format_host(fmt, data, abs_offset=n)
        same(c.wait(t2), expected(fmt, True, origin=n)[0], "second ticket")
        same(c.last_soft(), rows, "second ticket rows")
        same(c.wait(t1), want, "first ticket")
        same(c.last_soft(), rows, "first ticket rows")
    # device-resident: blocking and submitted, another rule
    rule = dict(n_weak=16, max_flips=5, min_key=0.0)
    want16, rows16 = expected(fmt, True, rule)
    assert (rows16["nflip"] > 0).sum() > soft.sum()
    c = make_ctx(S | F, fmt, rule)
    d = c.device_alloc(np.asarray(data).nbytes)
    try:
        c.device_upload(d, np.ascontiguousarray(data))
        same(c.process_format_device(fmt, d, n), want16, "process_format_device")
        same(c.last_soft(), rows16, "device rows")
        t = c.submit_format_device(fmt, d, n, abs_offset=7)
        with pytest.raises(N.AdsbError):
            c.set_soft_fec()                                         # -EBUSY while a ticket is pending
        same(c.wait(t), expected(fmt, True, rule, origin=7)[0], "submit_format_device")
        same(c.last_soft(), rows16, "submitted device rows")
        c.set_soft_fec()                                             # back to the defaults
        same(c.process_format_device(fmt, d, n), want, "defaults again")
    finally:
        c.device_free(d)


def test_small_passes_and_the_pinned_mirror(native):
    """A pass of one workgroup (records straight into pinned memory), a mid-size pass (the mirror beside the device list) and
    the whole stream: cut pieces of the float stream, each against the replay of its own flag-off records."""
    x = stream(N.FMT_MAG2)[1]
    for lo, hi in ((0, 1 << 12), (1 << 12, 1 << 16), (1 << 16, 1 << 19)):
        piece = np.ascontiguousarray(x[lo:hi])
        raw = make_ctx(0).process_format(N.FMT_MAG2, piece, abs_offset=lo)
        want, rows = SR.replay_records(raw, piece, lo, SPS, None, True)
        c = make_ctx(S | F)
        same(c.process_format(N.FMT_MAG2, piece, abs_offset=lo), want, (lo, hi))
        same(c.last_soft(), rows, (lo, hi))
    assert (rows["nflip"] > 0).sum() >= 5


def test_demod_work_slices(native):
    x = stream(N.FMT_MAG2)[1]
    raw = raw_records(N.FMT_MAG2)
    tags = raw["offset"][(raw["flags"] & N.BURST_DEMOD) != 0]
    tags = np.concatenate([tags, [len(x) - 50]])                                   # and one tag whose burst leaves the chunk
    for flags in (S, S | F):
        c0 = make_ctx(flags & ~S)
        b0, _, _ = c0.demod_work(x, 0, tags)
        want_bits, want_ok, want_rows = SR.replay_slices(np.packbits(b0, axis=1), c0.last_demod_flags, tags, x, SPS)
        c = make_ctx(flags)
        b, ok, _ = c.demod_work(x, 0, tags)
        same(np.packbits(b, axis=1), want_bits, "bits")
        same(c.last_demod_flags, want_ok, "ok")
        same(c.last_soft(), want_rows, "rows")
        fixed = want_rows["nflip"] > 0
        assert fixed.sum() >= 10 and ((want_ok & 2) != 0)[fixed].all() and not ok[-1] and not want_rows[-1].tobytes().strip(b"\0")
        # the rows of the last call are the records' again after a pass
        c.process_format(N.FMT_MAG2, x[:1 << 14])
        assert len(c.last_soft()) == len(c.last_result())


def test_confidence_ratios_stay_those_of_the_raw_slice(native):
    data, x = stream(N.FMT_FC32)
    c0, c1 = make_ctx(N.FLAG_CONFIDENCE), make_ctx(N.FLAG_CONFIDENCE | S | F)
    c0.process_format(N.FMT_FC32, data)
    same(c1.process_format(N.FMT_FC32, data), expected(N.FMT_FC32, True)[0], "confidence context")
    assert c0.last_confidence().tobytes() == c1.last_confidence().tobytes()
    same(c1.last_soft(), expected(N.FMT_FC32, True)[1], "rows")


def test_table_and_decode_steps_see_the_repaired_reply(native):
    """With the aircraft table and the decode step, the rows equal adsb_decode_pdus over the repaired PDUs on a context
    without the flag, and the records' bits are the replay's."""
    data, x = stream(N.FMT_FC32)
    want, rows = expected(N.FMT_FC32, True)
    c = make_ctx(S | F | T | DEC)
    c.set_decoder("All Messages", START)
    recs = c.process_format(N.FMT_FC32, data)
    dec = c.last_decoded()
    same(c.last_soft(), rows, "rows")
    ap = np.uint16(N.BURST_AP_KNOWN | N.BURST_AP_FEC)
    assert np.array_equal(recs["bits"], want["bits"]) and np.array_equal(recs["flags"] & ~ap, want["flags"] & ~ap)
    dem = np.flatnonzero((recs["flags"] & N.BURST_DEMOD) != 0)
    ref = make_ctx(F | T | DEC)
    ref.set_decoder("All Messages", START)
    ref_rows = ref.decode_pdus(recs["bits"][dem], np.array([START + int(o) / FS for o in recs["offset"][dem]], dtype=np.float64))
    same(dec[dem], ref_rows, "decoded rows")
    soft = rows["nflip"][dem] > 0
    # (a reply that passes parity is still published only if the decoder handles its type: the rows above say which)
    assert soft.sum() >= 10 and (dec["port"][dem][soft] != N.DEC_NONE).any()
    # the same context without the soft flag publishes none of those replies
    plain = make_ctx(F | T | DEC)
    plain.set_decoder("All Messages", START)
    plain.process_format(N.FMT_FC32, data)
    assert (plain.last_decoded()["port"][dem][soft] == N.DEC_NONE).all()


def test_arguments_and_refusals(native):
    data, x = stream(N.FMT_MAG2)
    for bad in (N.FLAG_STREAM_DECODE, N.FLAG_FRAMER_SLICES):
        with pytest.raises(N.AdsbError):
            N.Context(FS, THR, flags=S | bad)
    plain = make_ctx(0)
    with pytest.raises(N.AdsbError):
        plain.set_soft_fec()
    with pytest.raises(N.AdsbError):
        plain.last_soft()
    c = make_ctx(S)
    for bad in (dict(n_weak=0), dict(n_weak=17), dict(max_flips=0), dict(max_flips=6), dict(min_key=-0.1), dict(min_key=1.5),
                dict(min_key=float("nan"))):
        with pytest.raises(N.AdsbError):
            c.set_soft_fec(**bad)
    rule = N.SOFT_FEC_RULE(8, 3, 0.0, 1)
    assert c.lib.adsb_set_soft_fec(c._h, rule) == -22
    c.set_soft_fec(n_weak=1, max_flips=1, min_key=1.0)
    c.set_soft_fec(n_weak=16, max_flips=5, min_key=0.0)
    assert len(c.last_soft()) == 0
    # the entry points that refuse confidence contexts refuse this one
    piece = np.ascontiguousarray(x[:1 << 14])
    with pytest.raises(N.AdsbError):
        c.process_batch(N.FMT_MAG2, [piece, piece])
    with pytest.raises(N.AdsbError):
        c.open_streams(2)
    d = c.device_alloc(piece.nbytes)
    try:
        c.device_upload(d, piece)
        with pytest.raises(N.AdsbError):
            c.process_sharded_device(N.FMT_MAG2, d, len(piece), 2)
        assert len(c.process_format_device(N.FMT_MAG2, d, len(piece))) == len(c.last_soft())
    finally:
        c.device_free(d)
    with pytest.raises(N.AdsbError):
        N.process_sharded_multi([make_ctx(S), make_ctx(S)], N.FMT_MAG2, piece, shards_per_ctx=1)


def test_demod_block_counts_soft_repairs(native):
    from gr_adsb_amd import blocks, grshim
    x = stream(N.FMT_MAG2)[1]
    sched = [1 << 15] * (len(x) >> 15)
    out = {}
    for name, kw in (("plain", {}), ("cons", dict(error_corr="Conservative")), ("both", dict(error_corr="Conservative", soft_fec=True))):
        fr = blocks.framer(FS, THR)
        dm = blocks.demod(FS, parity_filter=True, **kw)
        dm.start_timestamp = 0.0
        _, msgs = grshim.drive(fr, dm, x, sched)
        out[name] = (dm, [bytes(np.asarray(m[1], dtype=np.uint8)) for _, m in msgs])
    plain, cons, both = out["plain"], out["cons"], out["both"]
    assert plain[0].soft_corrected == cons[0].soft_corrected == 0 and plain[0].corrected == 0
    assert both[0].corrected == cons[0].corrected >= 1 and both[0].soft_corrected >= 10
    assert len(both[1]) == len(cons[1]) + both[0].soft_corrected and len(cons[1]) >= len(plain[1]) + cons[0].corrected
    assert set(cons[1]) <= set(both[1])
