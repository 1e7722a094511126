"""Opt-in Conservative error correction on the MI355X (ADSB_FLAG_FEC_CONSERVATIVE): a stream built from every row of
tests/golden/g_fec.npz (modulator.burst_waveform, high SNR) through every entry point that returns records.  A FEC
context's records equal adsb_mode_s_fec applied to a flag-off context's records, every other field identical; the
repaired bits are the reference decoder's; flag-off records carry the raw bits.  The demod block's error_corr option
publishes what a Conservative decoder can accept, stand-alone and paired.  The CPU half is tests/test_fec.py."""
import numpy as np
import pytest

from gr_adsb_amd import _native as N
from gr_adsb_amd import modulator as M
from test_fec import FEC_BITS, GOLDEN, PI, expected_fec

pytestmark = pytest.mark.gpu

SPACING_US = 200                 # one reply (120 us) per 200 us: a false tag inside a reply (gate 63 us) never hides the next row
THR = 0.05
FMTS = {"fc32": N.FMT_FC32, "sc16": N.FMT_SC16, "sc8": N.FMT_SC8}


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_streams = {}


def stream(golden, fs):
    """(complex64 IQ, burst start of every row): the rows one after another, amplitude 1 over AWGN at -40 dB."""
    if fs not in _streams:
        sps = int(fs // 1e6)
        rows = np.unpackbits(golden["bits"], axis=1)[:, :112]
        step = SPACING_US * sps
        starts = 200 * sps + step * np.arange(len(rows))
        rng = np.random.default_rng(int(fs))
        n = int(starts[-1] + step + 400 * sps)
        z = ((rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) *
             np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
        for s, b in zip(starts, rows):
            env = M.burst_waveform(b, sps)
            z[s:s + len(env)] += env
        _streams[fs] = (z, starts)
    return _streams[fs]


def host_data(fmt, iq):
    if fmt == N.FMT_FC32:
        return iq
    if fmt == N.FMT_SC16:
        return M.quantize_iq16(iq)
    return M.quantize_iq8(iq)


def scale_of(fmt):
    return {N.FMT_SC16: 2.0 / 32767.0, N.FMT_SC8: 2.0 / 127.0}.get(fmt)


def make_ctx(fs, flags, fmt=None):
    c = N.Context(fs, THR, flags=flags)
    if fmt is not None and scale_of(fmt):
        c.set_format_scale(fmt, scale_of(fmt))
    return c


def rows_of(recs, starts, sps):
    """Index of the record of every row (its tag lies within a chip of the burst start)."""
    off = recs["offset"]
    i = np.searchsorted(off, starts - sps)
    assert (i < len(off)).all()
    assert (np.abs(off[i] - starts) <= sps).all(), "a row has no record"
    return i


def check_pair(off, on, golden, starts, sps, what):
    """FEC records == mode_s_fec(flag-off records); raw bits in flag-off records; the reference's repairs in FEC ones."""
    assert len(off) == len(on), what
    assert (off["flags"] & FEC_BITS == 0).all(), what
    want = expected_fec(off)
    assert on.tobytes() == want.tobytes(), what
    dem = (off["flags"] & N.BURST_DEMOD) != 0
    if starts is None:
        return int(np.count_nonzero(on["flags"] & N.BURST_FEC_FIXED))
    i = rows_of(off, starts, sps)
    assert dem[i].all(), what
    assert np.array_equal(off["bits"][i], golden["bits"]), what + ": raw slice differs from the rows"
    fl = on["flags"][i]
    fixed = (fl & N.BURST_FEC_FIXED) != 0
    assert np.array_equal(on["bits"][i][fixed], golden["bits_all"][fixed]), what
    assert np.array_equal(on["bits"][i][~fixed], golden["bits"][~fixed]), what
    df0 = golden["df0_all"]
    repaired_by_ref = (golden["bits_all"] != golden["bits"]).any(axis=1) & np.isin(df0, PI)
    assert np.array_equal(fixed | ((fl & N.BURST_FEC_DF) != 0), repaired_by_ref), what
    return int(fixed.sum())


@pytest.mark.parametrize("fs", [2e6, 8e6])
@pytest.mark.parametrize("fmt_name", list(FMTS))
def test_fec_records_every_entry_point(native, golden, fs, fmt_name):
    fmt = FMTS[fmt_name]
    sps = int(fs // 1e6)
    iq, starts = stream(golden, fs)
    data = host_data(fmt, iq)
    n = len(iq)
    F = N.FLAG_FEC_CONSERVATIVE
    # blocking, host-fed
    off = make_ctx(fs, 0, fmt).process_format(fmt, data)
    on = make_ctx(fs, F, fmt).process_format(fmt, data)
    assert check_pair(off, on, golden, starts, sps, "process_format") > 700
    # submitted / waited: the tail on the pass's own stream, and (timed context) on a second stream behind an event
    for extra in (0, N.FLAG_TIMING):
        res = []
        for fl in (extra, extra | F):
            c = make_ctx(fs, fl, fmt)
            t1 = c.submit_format_host(fmt, data)
            t2 = c.submit_format_host(fmt, data, abs_offset=n)
            res.append((c.wait(t1), c.wait(t2)))
        check_pair(res[0][0], res[1][0], golden, starts, sps, "submit/wait %d" % extra)
        check_pair(res[0][1], res[1][1], golden, starts + n, sps, "submit/wait second %d" % extra)
    # device memory: blocking, sharded driver, one shard
    res = []
    for fl in (0, F):
        c = make_ctx(fs, fl, fmt)
        d = c.device_alloc(np.asarray(data).nbytes)
        try:
            c.device_upload(d, np.ascontiguousarray(data))
            r_dev = c.process_format_device(fmt, d, n)
            r_sh = c.process_sharded_device(fmt, d, n, 4)
            lo, hi = int(n // 3), int(2 * n // 3)
            r_one = c.shard_device(fmt, d, n, 0, lo, hi, n, head_cands=0)
        finally:
            c.device_free(d)
        res.append((r_dev, r_sh, r_one))
    check_pair(res[0][0], res[1][0], golden, starts, sps, "process_format_device")
    check_pair(res[0][1], res[1][1], golden, starts, sps, "process_sharded_device")
    assert check_pair(res[0][2], res[1][2], golden, None, sps, "shard_device") > 100
    # one process, two contexts on this device
    res = []
    for fl in (0, F):
        cs = [make_ctx(fs, fl, fmt) for _ in range(2)]
        res.append(N.process_sharded_multi(cs, fmt, data, shards_per_ctx=2))
    check_pair(res[0], res[1], golden, starts, sps, "process_sharded_multi")
    mixed = [make_ctx(fs, 0, fmt), make_ctx(fs, F, fmt)]
    with pytest.raises(N.AdsbError):
        N.process_sharded_multi(mixed, fmt, data, shards_per_ctx=1)


def framer_calls(c, x, sps, N_chunk):
    H = 8 * sps
    buf = np.concatenate([np.zeros(H - 1, dtype=np.float32), x])
    out = []
    for pos in range(0, len(x), N_chunk):
        Nc = min(N_chunk, len(x) - pos)
        out.append(c.framer_work(buf[pos:pos + Nc + H - 1], Nc, pos))
    return np.concatenate(out)


@pytest.mark.parametrize("fs", [2e6, 8e6])
def test_fec_framer_slices_and_demod_work(native, golden, fs):
    sps = int(fs // 1e6)
    iq, starts = stream(golden, fs)
    x = M.mag2(iq)
    F = N.FLAG_FEC_CONSERVATIVE
    res = [framer_calls(N.Context(fs, THR, flags=N.FLAG_FRAMER_SLICES | fl), x, sps, 1 << 16) for fl in (0, F)]
    # (the reference framer's chunk-boundary behaviour -- stale gate state, framer.py:177-179; pulses high at a call's end,
    # :102-108; bursts that straddle it come back without bits -- costs this chunking a share of the rows: not every row)
    assert check_pair(res[0], res[1], golden, None, sps, "framer_work") > 300
    # demod_work: the tags of every row, one call over the whole stream and calls of 2^16 samples
    for chunk in (len(x), 1 << 16):
        outs = []
        for fl in (0, F):
            c = N.Context(fs, 0.0, flags=fl)
            bits, oks, flags = [], [], []
            for pos in range(0, len(x), chunk):
                m = (starts >= pos) & (starts < pos + chunk)
                b, _, _ = c.demod_work(x[pos:pos + chunk], pos, starts[m])
                bits.append(b); flags.append(N.demod_flags(c.last_demod_flags))
            outs.append((np.concatenate(bits), np.concatenate(flags)))
        (b0, f0), (b1, f1) = outs
        rec = np.zeros(len(b0), dtype=N.BURST_DTYPE)
        rec["bits"] = np.packbits(b0, axis=1)
        rec["flags"] = np.where(f0 & N.BURST_DEMOD, f0 | [N.mode_s_syndrome(b)[1] << 8 for b in rec["bits"]], 0)
        want = expected_fec(rec)
        ok = (f0 & N.BURST_DEMOD) != 0
        assert ok.mean() > 0.9 and (f0 & FEC_BITS == 0).all()
        assert np.array_equal(np.packbits(b1, axis=1), want["bits"])
        assert np.array_equal(f1, want["flags"] & ~np.uint16(0x1F00))
        if chunk == len(x):
            assert ok.all() and np.array_equal(rec["bits"], golden["bits"])


@pytest.mark.parametrize("paired", [False, True])
def test_conservative_demod_block_publishes_what_the_decoder_accepts(native, golden, paired):
    from gr_adsb_amd import blocks, grshim
    fs = 2e6
    iq, starts = stream(golden, fs)
    x = M.mag2(iq)
    sched = [1 << 15] * (len(x) >> 15) + ([len(x) & ((1 << 15) - 1)] if len(x) & ((1 << 15) - 1) else [])
    # the reference blocks' PDUs (error_corr="None", no filter) ...
    fr = blocks.framer(fs, THR)
    dm = blocks.demod(fs, framer=fr if paired else None)
    dm.start_timestamp = 0.0
    _, raw = grshim.drive(fr, dm, x, sched)
    # ... and what a Conservative decoder can accept of them, repaired as the device repairs them
    want = []
    for _, m in raw:
        b14 = np.packbits(np.asarray(m[1], dtype=np.uint8))
        v, rep, _, _ = N.mode_s_fec(b14)
        if blocks._prefilter_pass(v, int(v >> N.BURST_DF_SHIFT) & 31, True):
            want.append((m[0]["timestamp"], np.float32(m[0]["snr"]).tobytes(), bytes(np.unpackbits(rep)[:112]), bool(v & N.BURST_FEC_FIXED)))
    fr = blocks.framer(fs, THR)
    dm = blocks.demod(fs, framer=fr if paired else None, parity_filter=True, error_corr="Conservative")
    dm.start_timestamp = 0.0
    _, msgs = grshim.drive(fr, dm, x, sched)
    got = [(m[0]["timestamp"], np.float32(m[0]["snr"]).tobytes(), bytes(np.asarray(m[1], dtype=np.uint8))) for _, m in msgs]
    assert got == [w[:3] for w in want]
    assert dm.corrected == sum(w[3] for w in want) > 500
    assert dm.filtered == len(raw) - len(want) > 0


def test_confidence_ratios_stay_those_of_the_raw_slice(native, golden):
    """demod.py:101: bit_confidence belongs to the sliced samples, not to the repaired bits."""
    fs = 2e6
    iq, starts = stream(golden, fs)
    res = []
    for fl in (N.FLAG_CONFIDENCE, N.FLAG_CONFIDENCE | N.FLAG_FEC_CONSERVATIVE):
        c = make_ctx(fs, fl)
        recs = c.process_format(N.FMT_FC32, iq)
        res.append((recs, c.last_confidence()))
    check_pair(res[0][0], res[1][0], golden, starts, 2, "confidence context")
    assert res[0][1].tobytes() == res[1][1].tobytes()
    b = c.demod_work(M.mag2(iq), 0, starts, want_ratio=True)
    b0 = make_ctx(fs, 0).demod_work(M.mag2(iq), 0, starts, want_ratio=True)
    assert b[2].tobytes() == b0[2].tobytes()
