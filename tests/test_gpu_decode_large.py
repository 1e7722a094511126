"""The decode step on the MI355X with more keys than one workgroup of its sort takes (4096): adsb_decode_pdus in one call of
a tile + 1, of 13500 and of 80000 PDUs (20 workgroups: the scan's carry) and cut around a tile on one context; one
adsb_process_* pass whose list holds more than two tiles of demodulated records, under fc32 and sc8, repeated after
adsb_reset; three submissions in flight on a fresh context, the sort's buffers growing while a decode step is queued.
Expected rows: the plain-Python replay (tests/decode_replay.py).  The CPU half: tests/test_decode_sort.py and
test_emulated_kernels_over_several_sort_tiles in tests/test_decode.py."""
import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
from gr_adsb_amd import _native as N
from test_decode import BUSY, LARGE_CONFIGS, SORT_TILE, large_expected, large_stream
from test_gpu_decode import F, FMTS, THR, T, _scaled, dec_ctx, expect_rows, host_data, run_calls, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


def tile_cuts(n):
    cut = np.cumsum([0, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
    assert cut[-1] < n
    return list(zip(cut.tolist(), cut[1:].tolist() + [n]))


@pytest.mark.parametrize("filt,corr", LARGE_CONFIGS)
def test_decode_pdus_over_several_sort_tiles(native, filt, corr):
    b14, ts = large_stream()
    exp = large_expected(filt, corr)
    c = dec_ctx(filt, corr)
    n = SORT_TILE + 1                                  # two workgroups, the second with one key
    S.assert_rows_equal(c.decode_pdus(b14[:n], ts[:n]), exp[:n])
    c.reset()
    S.assert_rows_equal(c.decode_pdus(b14, ts), exp)   # the busy aircraft's segment crosses a tile boundary (large_expected)
    c.reset()
    got = np.concatenate([c.decode_pdus(b14[lo:hi], ts[lo:hi]) for lo, hi in tile_cuts(len(b14))])
    S.assert_rows_equal(got, exp)


def test_decode_pdus_of_more_than_sixteen_tiles(native):
    """80000 PDUs of 5000 aircraft in random order, more than 16 tiles of them with a key: 20 workgroups, a scan of 320 entries
    in two rounds; every aircraft's records lie tiles apart in the list and side by side after the sort."""
    filt, corr = "All Messages", "Conservative"
    addresses = [0, 0xFFFFFF] + [0x200000 + 2039 * k for k in range(4998)]
    b14, ts = S.mixed(np.random.default_rng(41), n=80000, addresses=addresses, dt=(0.002, 0.05))
    exp = S.to_rows(D.Decoder(filt, corr).rows(b14, ts))
    keyed = exp[(exp["present"] & N.DEC_HAS_PLANE) != 0]
    assert len(keyed) > 16 * SORT_TILE and len(set(keyed["icao"].tolist())) >= 4096
    first, last = {}, {}
    for i in np.flatnonzero((exp["present"] & N.DEC_HAS_PLANE) != 0):
        first.setdefault(int(exp["icao"][i]), i)
        last[int(exp["icao"][i])] = i
    assert sum(last[a] - first[a] > SORT_TILE for a in first) >= 4096
    c = dec_ctx(filt, corr)
    S.assert_rows_equal(c.decode_pdus(b14, ts), exp)
    c.reset()
    got = np.concatenate([c.decode_pdus(b14[lo:hi], ts[lo:hi]) for lo, hi in tile_cuts(len(b14))])
    S.assert_rows_equal(got, exp)


N_BURSTS = 10500
FS = 2e6


def dense_stream():
    """The first 10500 PDUs of large_stream (about 5400 of them the busy aircraft's) as one 2 Msps stream, 200 us apart."""
    b14, _ = large_stream()
    return stream(b14[:N_BURSTS], FS)


@pytest.mark.parametrize("fmt_name", ["fc32", "sc8"])
def test_one_pass_of_more_than_two_sort_tiles(native, fmt_name):
    """One call over the whole stream (whether the pass is re-run for list capacity: stats()["retries"], printed below)."""
    filt, corr = "All Messages", "Conservative"
    fmt = FMTS[fmt_name]
    iq, starts = dense_stream()
    data = host_data(fmt, iq)
    plain = N.Context(FS, THR, flags=T | F) if fmt == N.FMT_FC32 else _scaled(FS, T | F, fmt)
    ref = plain.process_format(fmt, data)
    c = dec_ctx(filt, corr, FS, fmt)
    recs = c.process_format(fmt, data)
    rows = c.last_decoded()
    print("one pass %s: %d records, %d demodulated, retries %d" % (fmt_name, len(recs), int((recs["flags"] & N.BURST_DEMOD != 0).sum()),
                                                                  c.stats()["retries"]))
    assert ((recs["flags"] & N.BURST_DEMOD) != 0).sum() > 2 * SORT_TILE
    assert recs.tobytes() == ref.tobytes()
    exp = expect_rows(recs, D.Decoder(filt, corr), FS)
    assert exp["num_msgs"][exp["icao"] == BUSY].max() > SORT_TILE
    S.assert_rows_equal(rows, exp)
    # adsb_reset: the same pass again gives the same rows
    c.reset()
    recs2 = c.process_format(fmt, data)
    assert recs2.tobytes() == recs.tobytes() and c.last_decoded().tobytes() == rows.tobytes()


def test_sort_buffers_grow_behind_a_queued_decode_step(native):
    """A fresh context, three submissions in flight, waited for newest first: a short pass, then two of more than a tile of
    records each, so that launch_dec enlarges the key, sorted-key and histogram buffers while the decode step before is
    still queued.  The rows equal the replay carried across the three."""
    filt, corr = "All Messages", "Conservative"
    iq, starts = dense_stream()
    sps = int(FS // 1e6)
    at = [0, int(starts[150]) - 40 * sps, int(starts[150 + 5100]) - 40 * sps, len(iq)]
    spans = list(zip(at[:-1], at[1:]))
    c = dec_ctx(filt, corr, FS)
    recs, rows = run_calls(c, N.FMT_FC32, iq, spans, submit=True)
    assert len(recs) == 3 and len(recs[0]) < 200
    rep = D.Decoder(filt, corr)
    for r, d in zip(recs, rows):
        S.assert_rows_equal(d, expect_rows(r, rep, FS))
    assert all(((r["flags"] & N.BURST_DEMOD) != 0).sum() > SORT_TILE for r in recs[1:])
    ref, _ = run_calls(N.Context(FS, THR, flags=T | F), N.FMT_FC32, iq, spans, decoded=False)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(recs, ref))
