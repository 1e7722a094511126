"""Plane snapshots on the MI355X (adsb_planes, adsb_stream_planes: the k_planes_* kernels behind the host code of
adsb_hip.hip): the rows equal the plain-Python replay's planes (tests/decode_replay.py) and tests/golden/g_planes.npz -- the
reference decoder's plane_dict --, a snapshot changes nothing, the refusals, blocks.decoder.plane_dict / plane_table and
frontend.Receivers.planes.  The CPU half (emulator, the golden itself) is tests/test_planes.py.  Nothing here reads the
reference tree."""
import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from gr_adsb_amd import modulator as M
from test_decode import seq_slices
from test_gpu_decode import THR, stream
from test_gpu_stream_decode import CU8_SCALE, FS, expect_rows
from test_planes import CHUNK, TOP, check_against_golden, golden_of, ident, plane_rows, rows_equal

pytestmark = pytest.mark.gpu

T, F, DEC, SD = N.FLAG_AIRCRAFT_TABLE, N.FLAG_FEC_CONSERVATIVE, N.FLAG_DECODE, N.FLAG_STREAM_DECODE
ENOSPC, EINVAL, EBUSY = 28, 22, 16


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


def planes_rc(ctx, cap):
    """adsb_planes with a buffer of exactly cap rows: (rc, n_out, rows with a guard row behind them)"""
    import ctypes
    rows = np.zeros(cap + 1, dtype=N.DECODED_DTYPE)
    rows.view(np.uint8)[:] = 0xA5
    n = ctypes.c_int32(-1)
    rc = ctx.lib.adsb_planes(ctx._h, ctypes.c_void_p(rows.ctypes.data), cap, ctypes.byref(n))
    return rc, n.value, rows


# ---- one decoder -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", ["None", "Conservative"])
def test_planes_equal_the_replay(native, corr):
    """3000 PDUs of 404 aircraft -- addresses 0 and 0xFFFFFF and a pair on each side of a scan chunk's boundary among them --
    through decode_pdus: the snapshot is the replay's planes in address order; a second one is identical; 600 PDUs decoded
    afterwards give the replay's rows and the next snapshot its planes; one row short is -ENOSPC with the count and an
    untouched buffer; after reset() there is nothing."""
    filt = "All Messages"
    addr = [0, 0xFFFFFF, CHUNK - 1, CHUNK] + [0x400000 + 523 * k for k in range(400)]
    b, t = S.mixed(np.random.default_rng(51), n=3000, addresses=addr)
    b1, t1 = S.mixed(np.random.default_rng(52), n=600, addresses=addr[::3] + [0x123456, TOP - CHUNK - 1, TOP - CHUNK], t0=float(t[-1]) + 1)
    c = N.Context(2e6, THR, flags=T | DEC | (F if corr == "Conservative" else 0))
    c.set_decoder(filt, 0.0)
    rep = D.Decoder(filt, corr)
    assert len(c.planes()) == 0
    S.assert_rows_equal(c.decode_pdus(b, t), rep.rows(b, t))
    exp = plane_rows(rep.planes)
    assert len(exp) > 350 and {0, 0xFFFFFF, CHUNK - 1, CHUNK} <= set(exp["icao"].tolist())
    got = c.planes()
    rows_equal(got, exp)
    assert c.planes(cap=len(exp) + 5).tobytes() == got.tobytes() == c.planes(cap=3).tobytes()
    # one row short
    rc, n, buf = planes_rc(c, len(exp) - 1)
    assert rc == -ENOSPC and n == len(exp) and (buf.view(np.uint8) == 0xA5).all()
    rc, n, buf = planes_rc(c, len(exp))
    assert rc == 0 and n == len(exp) and buf[:n].tobytes() == got.tobytes() and (buf[n:].view(np.uint8) == 0xA5).all()
    # the decoder goes on as if nobody had looked
    S.assert_rows_equal(c.decode_pdus(b1, t1), rep.rows(b1, t1))
    later = plane_rows(rep.planes)
    assert len(later) >= len(exp) + 3
    rows_equal(c.planes(), later)
    c.reset()
    assert len(c.planes()) == 0
    rep = D.Decoder(filt, corr)
    S.assert_rows_equal(c.decode_pdus(b1, t1), rep.rows(b1, t1))
    rows_equal(c.planes(), plane_rows(rep.planes))
    c.close()


def test_planes_refusals(native):
    """-EINVAL without the flag and for bad arguments; -EBUSY while a submitted ticket is pending (adsb_submit_* is legal on
    ADSB_FLAG_DECODE and on ADSB_FLAG_STREAM_DECODE contexts, so both calls can meet one)."""
    import ctypes
    b14, _ = S.mixed(np.random.default_rng(53), n=60, addresses=[0x111111, 0x222222])
    iq, _ = stream(b14, FS)
    for flags in (0, T, SD):
        c = N.Context(FS, THR, flags=flags)
        assert _code(c.planes) == -EINVAL
        c.close()
    c = N.Context(FS, THR, flags=T | DEC)
    n = ctypes.c_int32(0)
    assert c.lib.adsb_planes(c._h, None, 4, ctypes.byref(n)) == -EINVAL and c.lib.adsb_planes(c._h, None, -1, ctypes.byref(n)) == -EINVAL
    assert c.lib.adsb_planes(c._h, None, 0, None) == -EINVAL
    assert _code(c.stream_planes) == -EINVAL                     # not a fleet
    tk = c.submit_format_host(N.FMT_FC32, iq)
    assert _code(c.planes) == -EBUSY
    assert len(c.wait(tk)) > 40
    assert len(c.planes()) == 2
    c.close()
    c = N.Context(FS, THR, flags=SD)
    assert _code(c.stream_planes) == -EINVAL                     # no streams yet
    c.open_streams(3)
    tk = c.submit_format_host(N.FMT_FC32, iq)
    assert _code(c.stream_planes) == -EBUSY
    c.wait(tk)
    rows, first = c.stream_planes()
    assert len(rows) == 0 and list(first) == [0, 0, 0, 0]
    for sel in ([1, 1], [2, 0], [0, 3], [-1]):
        with pytest.raises(ValueError):
            c.stream_planes(sel)
        s = np.array(sel, np.int32)
        f = np.zeros(len(sel) + 1, np.int32)
        assert c.lib.adsb_stream_planes(c._h, ctypes.c_void_p(s.ctypes.data), len(sel), None, 0, ctypes.c_void_p(f.ctypes.data),
                                        ctypes.byref(n)) == -EINVAL
    c.close_streams()
    assert _code(c.stream_planes) == -EINVAL
    c.close()


def test_planes_equal_the_reference_plane_dict(native):
    """The g_decode sequences under "All Messages" / "Conservative", each in a fresh decoder: the snapshot is the golden's
    plane_dict; through blocks.decoder: plane_dict has the reference's entries (types included) and plane_table its lines."""
    from gr_adsb_amd import blocks
    from test_planes import FIELDS, GOLD, TYPES
    from test_decode import GOLD as GOLD_DECODE
    g, gp = np.load(GOLD_DECODE), np.load(GOLD)
    tag, filt, corr = "all_cons", "All Messages", "Conservative"
    blk = blocks.decoder(filt, corr, "Brief")
    sls = seq_slices(g["seq"])
    n = 0
    for seq, sl in enumerate(sls):
        blk.reset()
        pdus = [({"timestamp": float(g["ts"][i]), "snr": float(g["snr"][i])}, np.unpackbits(g["bits"][i])) for i in range(sl.start, sl.stop)]
        blk.decode_pdus(pdus)
        e = golden_of(gp, tag, seq)
        check_against_golden(blk._ctx.planes(), e, seq)
        pd = blk.plane_dict
        assert list(pd) == ["{:06x}".format(int(a)) for a in e["icao"]]
        for i, d in enumerate(pd.values()):
            assert tuple(d) == FIELDS
            assert [type(d[k]) for k in FIELDS] == [TYPES[int(c)] for c in e["types"][i]]
            assert D.f64bits(d["speed"]) == int(e["speed"][i]) and D.f64bits(d["latitude"]) == int(e["lat"][i])
            assert d["num_msgs"] == int(e["nmsgs"][i])
        assert blk.plane_table(float(g["ts"][sl.stop - 1])) == [str(x) for x in e["line"]]
        n += len(pd)
    assert n > 150
    with pytest.raises(AttributeError):
        blk.plane_dict = {}
    blk.stop()


# ---- the fleet ---------------------------------------------------------------------------------------------------------------
def test_receivers_planes_equal_the_replays(native):
    """Six receivers on cu8 with the Conservative repair, about 200 replies each of 40 shared aircraft, pushed in three calls of
    uneven chunks; stream 2 is reset after the second call, stream 4 gets an END item in it: every stream's planes are those of
    a replay fed the stream's delivered records; a subset is the matching slice; the rows afterwards are unchanged."""
    filt, corr = "All Messages", "Conservative"
    addr = [0, 0xFFFFFF] + [0x480000 + 977 * k for k in range(38)]
    starts = [1760000000.625 + 0.37 * s for s in range(6)]
    srcs = []
    for s in range(6):
        b14, _ = S.mixed(np.random.default_rng(500 + s), n=200, addresses=addr)
        srcs.append(M.quantize_iq8(stream(b14, FS)[0], offset_binary=True))
    fe = frontend.FrontEnd(FS, THR, flags=SD | F)
    fe.ctx.set_format_scale(N.FMT_CU8, CU8_SCALE)
    rx = fe.receivers(6, fmt=N.FMT_CU8, starts=starts, msg_filter=filt)
    reps = [D.Decoder(filt, corr) for _ in range(6)]
    ns = [len(x) // 2 for x in srcs]
    cut = [[0, (n * (2 + s)) // 11, (n * (5 + s)) // 13, n] for s, n in enumerate(ns)]

    def feed(ids, out):
        for i, r, d in zip(ids, out, rx.rows):
            rows_equal(d, expect_rows(r, reps[i], starts[i]))

    def check(ids=None):
        got = rx.planes(ids)
        for i, rows in zip(range(6) if ids is None else ids, got):
            rows_equal(rows, plane_rows(reps[i].planes))
        return got

    assert [len(x) for x in rx.planes()] == [0] * 6
    for k in range(3):
        ids = [0, 1, 2, 3, 4, 5] if k != 1 else [5, 3, 4, 1, 2]                 # (call 2 leaves stream 0 out)
        parts = [srcs[i][2 * cut[i][k]:2 * cut[i][k + 1]] for i in ids]
        if k == 1:
            recs, first = rx.ctx.process_stream_batch(N.FMT_CU8, ids, parts, end=[i == 4 for i in ids])
            d = rx.ctx.last_stream_decoded()
            rx.rows = [d[first[j]:first[j + 1]] for j in range(len(ids))]
            feed(ids, [recs[first[j]:first[j + 1]] for j in range(len(ids))])
            assert rx.state(4)[0] == 0 and len(reps[4].planes) > 20           # ended, and its aircraft are still there
            full = check()
            rx.ctx.reset_stream(2)
            reps[2] = D.Decoder(filt, corr)
            assert len(full[2]) > 20 and len(check()[2]) == 0
        else:
            feed(ids, rx.push(parts, ids=ids))
            check()
    feed(range(6), rx.finish())
    full = check()
    assert 0 < len(full[2]) and sum(len(x) for x in full) > 200
    assert len(full[4]) > 20
    assert fe.ctx.stream_decoder_stats()[0] == sum(len(x) for x in full)
    for sel in ([3], [0, 5], [1, 2, 4]):
        got = check(sel)
        assert [x.tobytes() for x in got] == [full[i].tobytes() for i in sel]
    rows, first = fe.ctx.stream_planes()
    assert rows.tobytes() == np.concatenate(full).tobytes() and first[-1] == len(rows)
    rx.close()
    fe.ctx.close()
    plain = N.Context(FS, THR)
    with pytest.raises(ValueError):
        frontend.Receivers(plain, 2).planes()
    plain.close()


def test_fleet_snapshot_through_growth_and_a_sort_of_several_tiles(native):
    """64 receivers, 79 aircraft each, into a store reserved at its minimum: about 5000 planes, several growths, a key sort over two
    tiles.  The snapshot is the replays' planes."""
    import ctypes
    filt, corr, n_s = "Extended Squitter Only", "None", 64
    rng = np.random.default_rng(54)
    addr = [0, 0xFFFFFF] + [0x600000 + 8191 * k for k in range(77)]
    b14 = np.array([ident(a, rng) for a in addr], np.uint8)
    ctx = N.Context(FS, THR, flags=SD)
    ctx.open_streams(n_s)
    ctx.set_streams_decoder(filt)
    ctx.stream_decoder_reserve(256)
    reps = [D.Decoder(filt, corr) for _ in range(n_s)]
    iq = stream(b14, FS)[0]
    for lo in range(0, n_s, 16):                                             # 16 receivers a call, all of them hear the same samples
        ids = list(range(lo, lo + 16))
        recs, first = ctx.process_stream_batch(N.FMT_FC32, ids, [iq] * 16, end=True)
        d = ctx.last_stream_decoded()
        for j, i in enumerate(ids):
            rows_equal(d[first[j]:first[j + 1]], expect_rows(recs[first[j]:first[j + 1]], reps[i], 0.0))
    planes, cap, grows = ctx.stream_decoder_stats()
    per = [len(r.planes) for r in reps]
    assert planes == sum(per) and planes > 4096 + 500 and grows >= 3 and cap >= 2 * planes
    rows, first = ctx.stream_planes()
    assert len(rows) == planes and list(first) == [sum(per[:i]) for i in range(n_s + 1)]
    one = plane_rows(reps[0].planes)
    for i in range(n_s):
        rows_equal(rows[first[i]:first[i + 1]], plane_rows(reps[i].planes) if i % 9 == 0 else one)
    # one row short: the count, nothing written
    buf = np.zeros(planes, dtype=N.DECODED_DTYPE)
    buf.view(np.uint8)[:] = 0xA5
    n = ctypes.c_int32(0)
    assert ctx.lib.adsb_stream_planes(ctx._h, None, 0, ctypes.c_void_p(buf.ctypes.data), planes - 1, None, ctypes.byref(n)) == -ENOSPC
    assert n.value == planes and (buf.view(np.uint8) == 0xA5).all()
    sub, f2 = ctx.stream_planes([0, 31, 63])
    assert list(f2) == [0, per[0], per[0] + per[31], per[0] + per[31] + per[63]] and sub.tobytes() == np.concatenate([rows[first[i]:first[i + 1]] for i in (0, 31, 63)]).tobytes()
    ctx.close()
