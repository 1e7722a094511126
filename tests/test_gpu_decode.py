"""Opt-in decode step on the MI355X (ADSB_FLAG_DECODE): adsb_decode_pdus over every sequence of tests/golden/g_decode.npz
and g_decode_edges.npz under both msg_filter and error_corr values, whole and cut into pieces; adsb_process_* /
adsb_submit_* in three formats at two rates over a stream modulated from the golden rows, against the plain-Python replay (tests/decode_replay.py) of the
published records -- with calls cut between an aircraft's even and odd frames, three submissions waited for out of order,
adsb_reset, device memory; records byte-identical to a context without the flag; the refused entry points; blocks.decoder;
a stream with a new address in every burst over several passes.  The CPU half is tests/test_decode.py."""
import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
from gr_adsb_amd import _native as N
from gr_adsb_amd import modulator as M
from test_decode import CONFIGS, EDGES, GOLD, check_rows, expected, seq_slices

pytestmark = pytest.mark.gpu

T, F, DEC = N.FLAG_AIRCRAFT_TABLE, N.FLAG_FEC_CONSERVATIVE, N.FLAG_DECODE
THR = 0.05
SPACING_US = 200
FMTS = {"fc32": N.FMT_FC32, "sc16": N.FMT_SC16, "sc8": N.FMT_SC8}
START = 1760000000.625          # whole-second boundaries fall inside every stream below


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def dec_ctx(filt, corr, fs=2e6, fmt=None, extra=0):
    c = N.Context(fs, THR, flags=T | DEC | (F if corr == "Conservative" else 0) | extra)
    c.set_decoder(filt, START)
    if fmt is not None and fmt != N.FMT_FC32:
        c.set_format_scale(fmt, 2.0 / 32767.0 if fmt == N.FMT_SC16 else 2.0 / 127.0)
    return c


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_decode_pdus_equals_golden(native, g, tag, filt, corr):
    c = dec_ctx(filt, corr)
    sls = seq_slices(g["seq"])
    for piece in (None, 1, 7, 4096):
        got = np.zeros(len(g["bits"]), dtype=N.DECODED_DTYPE)
        for sl in sls:
            c.reset()
            step = piece or (sl.stop - sl.start)
            for lo in range(sl.start, sl.stop, step):
                hi = min(lo + step, sl.stop)
                got[lo:hi] = c.decode_pdus(g["bits"][lo:hi], g["ts"][lo:hi])
        check_rows(got, g, tag)


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_decode_pdus_equals_edges_golden(native, tag, filt, corr):
    """The NL zone edges on the CPR grid (tests/golden/g_decode_edges.npz): every sequence has its own address, so one call
    takes them all; then sequence by sequence."""
    ge = np.load(EDGES)
    c = dec_ctx(filt, corr)
    check_rows(c.decode_pdus(ge["bits"], ge["ts"]), ge, tag)
    c.reset()
    check_rows(np.concatenate([c.decode_pdus(ge["bits"][sl], ge["ts"][sl]) for sl in seq_slices(ge["seq"])]), ge, tag)


_streams = {}


def stream(bits14, fs):
    """complex64 IQ of the rows one after another (amplitude 1 over AWGN at -40 dB) and the burst starts."""
    key = (bits14.tobytes(), fs)
    if key not in _streams:
        sps = int(fs // 1e6)
        rows = np.unpackbits(bits14, axis=1)[:, :112]
        step = SPACING_US * sps
        starts = 200 * sps + step * np.arange(len(rows))
        rng = np.random.default_rng(int(fs) + 3)
        n = int(starts[-1] + step + 400 * sps)
        z = ((rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) *
             np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
        for s, b in zip(starts, rows):
            env = M.burst_waveform(b, sps)
            z[s:s + len(env)] += env
        _streams[key] = (z, starts)
    return _streams[key]


def host_data(fmt, iq):
    if fmt == N.FMT_FC32:
        return iq
    return M.quantize_iq16(iq) if fmt == N.FMT_SC16 else M.quantize_iq8(iq)


def piece(fmt, data, lo, hi):
    per = N.FMT_LAYOUT[fmt][1]
    return data[lo * per:hi * per]


def expect_rows(recs, rep, fs):
    """The rows a decode context writes for one call's records: the replay (carried across calls) for the records with
    BURST_DEMOD, in list order, at timestamps START + offset / fs; a fixed row for the others."""
    out = np.zeros(len(recs), dtype=N.DECODED_DTYPE)
    dem = np.flatnonzero((recs["flags"] & N.BURST_DEMOD) != 0)
    out[dem] = S.to_rows(rep.rows(recs["bits"][dem], [START + int(o) / fs for o in recs["offset"][dem]]))
    rest = np.setdiff1d(np.arange(len(recs)), dem)
    out["icao"][rest] = -1
    out["bits"][rest] = recs["bits"][rest]
    out["df"][rest] = recs["bits"][rest, 0] >> 3
    out["latitude"][rest] = out["longitude"][rest] = np.nan
    return out


def run_calls(c, fmt, data, spans, submit=False, decoded=True):
    recs, rows = [], []
    if not submit:
        for lo, hi in spans:
            recs.append(c.process_format(fmt, piece(fmt, data, lo, hi), abs_offset=lo))
            rows.append(c.last_decoded() if decoded else None)
        return recs, rows
    for k in range(0, len(spans), 3):
        tk = [c.submit_format_host(fmt, piece(fmt, data, lo, hi), abs_offset=lo) for lo, hi in spans[k:k + 3]]
        got = []
        for t in tk[::-1]:                         # waited for newest first: publication order is submission order
            got.append((c.wait(t), c.last_decoded()))
        for r, d in got[::-1]:
            recs.append(r)
            rows.append(d)
    return recs, rows


def check_calls(recs, rows, filt, corr, fs, what):
    rep = D.Decoder(filt, corr)
    n_dec = 0
    for k, (r, d) in enumerate(zip(recs, rows)):
        S.assert_rows_equal(d, expect_rows(r, rep, fs))
        n_dec += int((d["port"] == N.DEC_DECODED).sum())
    assert n_dec > 500, what
    return n_dec


def cuts(g, starts, sps, n):
    """Call boundaries between an aircraft's even and odd frames (the CPR pair sequences), and a few more."""
    bits = np.unpackbits(g["bits"], axis=1)
    tc = bits[:, 32:37].dot(1 << np.arange(4, -1, -1))
    df = bits[:, :5].dot(1 << np.arange(4, -1, -1))
    pos = np.flatnonzero((df == 17) & (tc == 11))
    at = sorted({int(starts[i + 1]) - 40 * sps for i in pos[::40] if i + 1 < len(starts)} | {int(starts[len(starts) // 2])})
    return [0] + at + [n]


@pytest.mark.parametrize("fs", [2e6, 8e6])
@pytest.mark.parametrize("fmt_name", list(FMTS))
def test_process_rows_equal_the_replay(native, g, fs, fmt_name):
    fmt = FMTS[fmt_name]
    sps = int(fs // 1e6)
    iq, starts = stream(g["bits"], fs)
    data = host_data(fmt, iq)
    n = len(iq)
    cs = cuts(g, starts, sps, n)
    spans = list(zip(cs[:-1], cs[1:]))
    assert len(spans) > 10 and int(START + n / fs) > int(START)
    for filt, corr in (("All Messages", "None"), ("All Messages", "Conservative"), ("Extended Squitter Only", "Conservative")):
        base = F if corr == "Conservative" else 0
        # flag-off table context: the records are byte-identical
        ref_recs, _ = run_calls(N.Context(fs, THR, flags=T | base) if fmt == N.FMT_FC32 else _scaled(fs, T | base, fmt),
                                fmt, data, spans, decoded=False)
        c = dec_ctx(filt, corr, fs, fmt)
        recs, rows = run_calls(c, fmt, data, spans)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(recs, ref_recs))
        check_calls(recs, rows, filt, corr, fs, "process %s %s" % (filt, corr))
        # adsb_reset: the same calls again give the same rows
        c.reset()
        recs2, rows2 = run_calls(c, fmt, data, spans)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, rows2))
        # three submissions in flight, waited for out of order
        c3 = dec_ctx(filt, corr, fs, fmt)
        recs3, rows3 = run_calls(c3, fmt, data, spans, submit=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(recs3, ref_recs))
        check_calls(recs3, rows3, filt, corr, fs, "submit %s %s" % (filt, corr))
        if fmt == N.FMT_FC32:
            # device memory, one call over the whole stream
            cd = dec_ctx(filt, corr, fs, fmt)
            d = cd.device_alloc(np.asarray(data).nbytes)
            try:
                cd.device_upload(d, np.ascontiguousarray(data))
                r = cd.process_format_device(fmt, d, n)
                check_calls([r], [cd.last_decoded()], filt, corr, fs, "device")
            finally:
                cd.device_free(d)


def _scaled(fs, flags, fmt):
    c = N.Context(fs, THR, flags=flags)
    c.set_format_scale(fmt, 2.0 / 32767.0 if fmt == N.FMT_SC16 else 2.0 / 127.0)
    return c


def test_refused_entry_points(native, g):
    fs, fmt = 2e6, N.FMT_FC32
    iq, starts = stream(g["bits"][:200], fs)
    n = len(iq)
    c = dec_ctx("All Messages", "None")
    x = M.mag2(iq)
    calls = [lambda: c.demod_work(x, 0, starts), lambda: c.framer_work(np.zeros(4096 + 15, np.float32), 4096, 0),
             lambda: c.shard_host(fmt, iq, 0, 0, n // 2, n)]
    for call in calls:
        with pytest.raises(N.AdsbError) as e:
            call()
        assert e.value.code == -22
    with pytest.raises(N.AdsbError):
        N.Context(fs, THR, flags=DEC)                              # without the table
    with pytest.raises(N.AdsbError):
        N.Context(fs, THR, flags=T).decode_pdus(g["bits"][:3], g["ts"][:3])   # without the decode flag
    assert len(c.process_format(fmt, iq)) > 150                  # the context itself still works


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_decoder_block_publishes_the_references_pdus(native, g, tag, filt, corr):
    from gr_adsb_amd import blocks
    blk = blocks.decoder(filt, corr, "Brief")
    exp = expected(g, tag)
    rep = S.to_rows([r for sl in seq_slices(g["seq"]) for r in D.Decoder(filt, corr).rows(g["bits"][sl], g["ts"][sl])])
    exp["velocity_we"], exp["velocity_sn"] = rep["velocity_we"], rep["velocity_sn"]
    assert blk.name() == "ADS-B Decoder"
    for sl in seq_slices(g["seq"]):
        blk.reset()
        for i in range(sl.start, sl.stop):
            meta = {"timestamp": float(g["ts"][i]), "snr": float(g["snr"][i])}
            n0 = len(blk.messages)
            blk._handlers["demodulated"]((meta, np.unpackbits(g["bits"][i])))
            new = blk.messages[n0:]
            want = N.decoded_pdu(exp[i], meta)
            if want is None:
                assert new == [], i
                continue
            assert len(new) == 1
            port, (d, vec) = new[0]
            assert port == want[0] and np.array_equal(vec, want[1][1])
            assert list(d) == list(want[1][0]) and all(type(d[k]) is type(want[1][0][k]) for k in d)
            assert all(D.f64bits(d[k]) == D.f64bits(want[1][0][k]) if isinstance(d[k], float) else d[k] == want[1][0][k] for k in d)
    assert blk.raised == int((g["port_" + tag] == 3).sum()) > 30
    assert sum(1 for p, _ in blk.messages if p == "decoded") == int((g["port_" + tag] == 1).sum())


def test_new_address_in_every_burst_over_several_passes(native):
    """Bench-like traffic: every burst a new address; several passes share one decoder state."""
    rng = np.random.default_rng(21)
    fs = 8e6
    b14, _ = S.mixed(rng, n=6000, addresses=[0x100000 + 7 * k for k in range(6000)])
    iq, starts = stream(b14, fs)
    n = len(iq)
    c = dec_ctx("All Messages", "Conservative", fs)
    spans = [(lo, min(lo + (1 << 21), n)) for lo in range(0, n, 1 << 21)]
    assert len(spans) >= 4
    recs, rows = run_calls(c, N.FMT_FC32, iq, spans)
    rep = D.Decoder("All Messages", "Conservative")
    icao = set()
    for r, d in zip(recs, rows):
        S.assert_rows_equal(d, expect_rows(r, rep, fs))
        icao |= set(d["icao"][(d["present"] & N.DEC_HAS_PLANE) != 0].tolist())
    assert len(icao) > 3000
