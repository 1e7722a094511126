"""Opt-in aircraft table on the MI355X (ADSB_FLAG_AIRCRAFT_TABLE): a stream built from every row of
tests/golden/g_aircraft.npz (modulator.burst_waveform, high SNR) through every entry point that publishes records.  A
flagged context's records equal a flag-off context's records (the same error_corr) plus the replay's BURST_AP_KNOWN /
BURST_AP_FEC (tests/aircraft_replay.py), every other byte identical -- with the calls cut so that announcements and the
replies of their addresses fall in different calls, with three submissions in flight waited for out of order, and after
adsb_reset.  The sharded entry points refuse a flagged context.  The demod block's msg_filter option publishes what the
decoder downstream accepts, stand-alone and improved, under four chunk schedules.  The CPU half is tests/test_aircraft.py."""
import numpy as np
import pytest

import aircraft_replay as A
from gr_adsb_amd import _native as N
from gr_adsb_amd import modulator as M
from test_aircraft import GOLDEN

pytestmark = pytest.mark.gpu

SPACING_US = 200                 # one reply (120 us) per 200 us, as in tests/test_gpu_fec.py
THR = 0.05
FMTS = {"fc32": N.FMT_FC32, "sc16": N.FMT_SC16, "sc8": N.FMT_SC8}
T, F = N.FLAG_AIRCRAFT_TABLE, N.FLAG_FEC_CONSERVATIVE


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
        rng = np.random.default_rng(int(fs) + 1)
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


def cuts(starts, sps, n):
    """Call boundaries 40 us ahead of a row: right after the announcement of a class row and before the replies of its
    address (the golden's sequences put the announcement second), and a few more."""
    at = [starts[1] - 40 * sps, starts[2] - 40 * sps, starts[7] - 40 * sps, starts[len(starts) // 2] - 40 * sps]
    return [0] + at + [n]


def piece(fmt, data, lo, hi):
    per = N.FMT_LAYOUT[fmt][1]
    return data[lo * per:hi * per]


def check(off_calls, on_calls, fec, what):
    """Flagged records == flag-off records + the replay's flags, call after call against one table."""
    known = set()
    n_known = n_fec = 0
    for k, (off, on) in enumerate(zip(off_calls, on_calls)):
        assert len(off) == len(on), (what, k)
        assert (off["flags"] & (N.BURST_AP_KNOWN | N.BURST_AP_FEC) == 0).all(), (what, k)
        want = A.expected_records(off, fec, known)
        assert on.tobytes() == want.tobytes(), (what, k)
        n_known += int(np.count_nonzero(on["flags"] & N.BURST_AP_KNOWN))
        n_fec += int(np.count_nonzero(on["flags"] & N.BURST_AP_FEC))
    assert n_known > 150, what
    assert (n_fec > 10) == fec, what
    return n_known


@pytest.mark.parametrize("fs", [2e6, 8e6])
@pytest.mark.parametrize("fmt_name", list(FMTS))
def test_table_every_entry_point(native, golden, fs, fmt_name):
    fmt = FMTS[fmt_name]
    sps = int(fs // 1e6)
    iq, starts = stream(golden, fs)
    data = host_data(fmt, iq)
    n = len(iq)
    cs = cuts(starts, sps, n)
    spans = list(zip(cs[:-1], cs[1:]))
    for base in (0, F):
        fec = base == F
        # blocking, host-fed, calls cut between announcements and replies; one flagged context throughout
        off_c, on_c = make_ctx(fs, base, fmt), make_ctx(fs, base | T, fmt)
        off = [off_c.process_format(fmt, piece(fmt, data, lo, hi), abs_offset=lo) for lo, hi in spans]
        on = [on_c.process_format(fmt, piece(fmt, data, lo, hi), abs_offset=lo) for lo, hi in spans]
        check(off, on, fec, "process_format %d" % base)
        # adsb_reset empties the table: the same calls again give the same flags
        on_c.reset()
        again = [on_c.process_format(fmt, piece(fmt, data, lo, hi), abs_offset=lo) for lo, hi in spans]
        check(off, again, fec, "after reset %d" % base)
        # three submissions in flight, waited for newest first: publication order is submission order
        for extra in (0, N.FLAG_TIMING):
            res = []
            for fl in (base | extra, base | extra | T):
                c = make_ctx(fs, fl, fmt)
                got = []
                for g in range(0, len(spans), 3):
                    tk = [c.submit_format_host(fmt, piece(fmt, data, lo, hi), abs_offset=lo) for lo, hi in spans[g:g + 3]]
                    got += [c.wait(t) for t in tk[::-1]][::-1]
                res.append(got)
            check(res[0], res[1], fec, "submit/wait %d %d" % (base, extra))
        # device memory
        res = []
        for fl in (base, base | T):
            c = make_ctx(fs, fl, fmt)
            d = c.device_alloc(np.asarray(data).nbytes)
            try:
                c.device_upload(d, np.ascontiguousarray(data))
                res.append([c.process_format_device(fmt, d, n), c.process_format_device(fmt, d, n, abs_offset=n)])
            finally:
                c.device_free(d)
        check(res[0], res[1], fec, "process_format_device %d" % base)


def test_sharded_entry_points_refuse_a_flagged_context(native, golden):
    fs, fmt = 2e6, N.FMT_FC32
    iq, _ = stream(golden, fs)
    n = len(iq)
    c = make_ctx(fs, T)
    d = c.device_alloc(iq.nbytes)
    try:
        c.device_upload(d, iq)
        for call in (lambda: c.process_sharded_device(fmt, d, n, 4),
                     lambda: c.shard_device(fmt, d, n, 0, 0, n // 2, n),
                     lambda: c.shard_host(fmt, iq, 0, 0, n // 2, n)):
            with pytest.raises(N.AdsbError) as e:
                call()
            assert e.value.code == -22
    finally:
        c.device_free(d)
    with pytest.raises(N.AdsbError):
        N.process_sharded_multi([make_ctx(fs, T), make_ctx(fs, T)], fmt, iq, shards_per_ctx=1)
    assert len(make_ctx(fs, T).process_format(fmt, iq)) > 1000          # the context itself still works


@pytest.mark.parametrize("fs", [2e6, 8e6])
def test_table_on_demod_work_slices(native, golden, fs):
    iq, starts = stream(golden, fs)
    x = M.mag2(iq)
    for base in (0, F):
        fec = base == F
        for chunk in (len(x), 1 << 16):
            outs = []
            for fl in (base, base | T):
                c = N.Context(fs, 0.0, flags=fl)
                bits, flags = [], []
                for pos in range(0, len(x), chunk):
                    m = (starts >= pos) & (starts < pos + chunk)
                    b, _, _ = c.demod_work(x[pos:pos + chunk], pos, starts[m])
                    bits.append(b)
                    flags.append(N.demod_flags(c.last_demod_flags))
                outs.append((np.concatenate(bits), np.concatenate(flags)))
            (b0, f0), (b1, f1) = outs
            assert np.array_equal(b0, b1)
            rec = np.zeros(len(b0), dtype=N.BURST_DTYPE)
            rec["bits"] = np.packbits(b0, axis=1)
            rec["flags"] = f0
            want = A.expected_records(rec, fec, set())["flags"]
            assert np.array_equal(f1, want), (base, chunk)
            assert int(np.count_nonzero(f1 & N.BURST_AP_KNOWN)) > 150


SCHED = ("single", "fixed4096", "fixed8192", "random")


def schedule(name, L, seed=7):
    if name == "single":
        return [L]
    if name.startswith("fixed"):
        k = int(name[5:])
        return [k] * (L // k) + ([L % k] if L % k else [])
    rng = np.random.default_rng(seed)
    out, left = [], L
    while left:
        k = min(left, int(rng.integers(500, 20000)))
        out.append(k)
        left -= k
    return out


@pytest.mark.parametrize("improved", [False, True])
@pytest.mark.parametrize("sched", SCHED)
def test_demod_block_publishes_what_the_decoder_accepts(native, golden, improved, sched):
    from gr_adsb_amd import blocks, grshim
    fs = 2e6
    iq, _ = stream(golden, fs)
    x = M.mag2(iq)
    s = schedule(sched, len(x))
    for corr in ("None", "Conservative"):
        fec = corr == "Conservative"
        fr = blocks.framer(fs, THR, improved=improved)
        dm = blocks.demod(fs, improved=improved, error_corr=corr)
        dm.start_timestamp = 0.0
        _, raw = grshim.drive(fr, dm, x, s)
        pub = np.array([np.packbits(np.asarray(m[1], dtype=np.uint8)) for _, m in raw])
        _, _, passed = A.replay(pub, fec)
        want = [(m[0]["timestamp"], bytes(np.asarray(m[1], dtype=np.uint8))) for (_, m), p in zip(raw, passed) if p]
        es = [(m[0]["timestamp"], bytes(np.asarray(m[1], dtype=np.uint8))) for (_, m), b in zip(raw, pub)
              if blocks._prefilter_pass(N.mode_s_fec(b)[0] if fec else _flags(b), int(b[0]) >> 3, fec,
                                        "Extended Squitter Only")]
        for mf, expect in (("All Messages", want), ("Extended Squitter Only", es)):
            fr = blocks.framer(fs, THR, improved=improved)
            dm = blocks.demod(fs, improved=improved, error_corr=corr, parity_filter=True, msg_filter=mf)
            dm.start_timestamp = 0.0
            _, msgs = grshim.drive(fr, dm, x, s)
            got = [(m[0]["timestamp"], bytes(np.asarray(m[1], dtype=np.uint8))) for _, m in msgs]
            assert got == expect, (corr, mf)
            assert dm.filtered == len(raw) - len(expect) > 0
        assert sum(1 for (_, m), p in zip(raw, passed) if p and int(np.packbits(m[1])[0]) >> 3 in A.AP_DFS) > 150


def _flags(b14):
    syn, df, nb = N.mode_s_syndrome(b14)
    f = (df << N.BURST_DF_SHIFT) | (N.BURST_LONG if nb == 112 else 0) | (N.BURST_KNOWN_DF if nb else 0)
    return f | (N.BURST_PARITY_OK if df in A.PI_DFS and syn == 0 else 0)
