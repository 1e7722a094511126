"""The fleet's merged picture on the MI355X (adsb_stream_planes_merged behind the host code of adsb_hip.hip):
tests/golden/g_merge.npz -- one reference decoder per stream and the table their plane_dicts fold into -- through both
stream-batch entry points; a fleet whose sorted keys exceed one sort tile, with segments across every seam of the kernels; three
streams in use out of 5000; the refusals, the untouched-state guarantees, an expiry between two merged calls and the buffers'
lifecycle.  The expectation is the golden's table, elsewhere test_merge.fold over the per-stream models that
test_gpu_expire.GpuFleet checks every decoded row against.  The CPU half (emulator, the golden itself, the fold) is
tests/test_merge.py.  Nothing here reads the reference tree."""
import ctypes

import numpy as np
import pytest

import test_planes as TP
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from test_expire import CONFIGS, INT64_MIN, ident
from test_gpu_decode import THR, stream
from test_gpu_expire import GpuFleet, pdu_iq
from test_gpu_stream_decode import FS
from test_merge import GOLD, SRC, Models, cases, check_case, fold, position, same, velocity

pytestmark = pytest.mark.gpu

T, F, DEC, SD, AGES = N.FLAG_AIRCRAFT_TABLE, N.FLAG_FEC_CONSERVATIVE, N.FLAG_DECODE, N.FLAG_STREAM_DECODE, N.FLAG_PLANE_AGES
ENOSPC, EINVAL, EBUSY = 28, 22, 16


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


@pytest.fixture(scope="module")
def gm():
    return np.load(GOLD)


def _code(fn, *a, **k):
    with pytest.raises(N.AdsbError) as e:
        fn(*a, **k)
    return e.value.code


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_golden_through_the_stream_batch(native, gm, tag, filt, corr, device):
    """The golden's five PDU lists as five receivers.  Every PDU is a modulated chunk of its own that ends its stream, the
    stream's start putting the PDU's clock where the golden has it; call k holds the k-th PDU of every stream that still has
    one.  Every stored selection and cutoff: rows and info byte-equal to the stored table."""
    import torch
    n = int(gm["n_streams"])
    c = N.Context(FS, THR, flags=SD | AGES | (F if corr == "Conservative" else 0))
    c.open_streams(n)
    c.set_streams_decoder(filt)
    lists = [np.flatnonzero(gm["stream"] == s) for s in range(n)]
    keep = []
    for k in range(max(len(x) for x in lists)):
        ids = [s for s in range(n) if k < len(lists[s])]
        chunks = [pdu_iq(gm["bits"][lists[s][k]]) for s in ids]
        for s in ids:
            c.set_stream_start(s, float(gm["ts"][lists[s][k]]) - 400 / FS)
        if device:
            dev = [torch.from_numpy(x.view(np.float32).copy()).cuda() for x in chunks]
            keep.append(dev)
            recs, first = c.process_stream_batch_device(N.FMT_FC32, ids, [d.data_ptr() for d in dev], [len(x) for x in chunks], end=True)
        else:
            recs, first = c.process_stream_batch(N.FMT_FC32, ids, chunks, end=True)
        assert first.tolist() == list(range(len(ids) + 1)), (k, first)              # one record per chunk
        for j, s in enumerate(ids):
            ts = (float(gm["ts"][lists[s][k]]) - 400 / FS) + int(recs["offset"][j]) / FS
            assert int(ts) == int(gm["ts"][lists[s][k]])                             # the decoder's clock is the golden's
    for case, sel, cutoff in cases(gm):
        check_case(c.merged_planes(sel, cutoff), gm, tag, case)
    assert c.merged_planes(None, None)[1].tobytes() == c.merged_planes(list(range(n)), INT64_MIN)[1].tobytes()
    c.close()


class Fleet(GpuFleet):
    """test_gpu_expire.GpuFleet whose per-stream models are made on first use"""

    class Lazy:
        def __init__(self, filt, corr):
            self.m = Models(filt, corr)

        def planes(self):
            return sum(len(m.d.planes) for m in self.m.values())

    def __init__(self, n, filt="All Messages", corr="None", slots=256):
        self.fe = frontend.FrontEnd(FS, THR, flags=SD | AGES | (F if corr == "Conservative" else 0))
        self.rx = self.fe.receivers(n, fmt=N.FMT_FC32, msg_filter=filt, ages=True)
        self.ctx = self.fe.ctx
        self.ctx.stream_decoder_reserve(slots)
        self.mod = Fleet.Lazy(filt, corr)

    def merged(self, ids=None, cutoff=None):
        return self.rx.merged(ids, cutoff)

    def check(self):
        for s, (rows, seen) in enumerate(self.rx.planes(seen=True)):
            erows, eseen = self.mod.m[s].snapshot()
            TP.rows_equal(rows, erows)
            assert np.array_equal(seen, eseen)
        assert self.ctx.stream_decoder_stats()[0] == self.mod.planes()

    def fold(self, ids, cutoff=INT64_MIN):
        return fold(self.mod.m, ids, cutoff)


def replies(addrs, rng):
    """One or two replies per aircraft: an identification, a velocity, one position frame (an altitude), a pair (a fix)"""
    out = []
    for a in addrs:
        kind = int(rng.integers(0, 5))
        if kind == 0:
            out += [ident(a, rng)]
        elif kind == 1:
            out += [velocity(a, rng)]
        elif kind == 2:
            out += [position(a, int(rng.integers(0, 2)), 40.0, 5.0, rng)]
        elif kind == 3:
            lat, lon = float(rng.uniform(-60, 60)), float(rng.uniform(-170, 170))
            out += [position(a, 0, lat, lon, rng), position(a, 1, lat, lon, rng)]
        else:
            out += [ident(a, rng), velocity(a, rng)]
    return out


def test_segments_across_every_seam(native):
    """test_merge.test_segments_across_every_seam's fleet on the device: 70 receivers x 60 shared aircraft and 22 aircraft of one
    receiver each, 4222 sorted keys -- more than one sort tile; segments across sorted rows 63 / 64, 255 / 256 and 4095 / 4096,
    two heads on either side of 511 / 512 (the placements are asserted there, from the key arithmetic; the addresses are the
    same).  The receivers hear in two rounds at whole seconds out of a handful, so that last_seen ties are common."""
    rng = np.random.default_rng(91)
    n, shared = 70, [0x100000 + 64 * i for i in range(60)]
    pads = {}
    for k in range(22):
        pads.setdefault(int(7 * k % n), []).append(shared[6] + 1 + k)
    f = Fleet(n, slots=16384)
    f.hear({s: (replies(shared[:30], rng), 5000.5 + s % 4) for s in range(n)})
    f.hear({s: (replies(shared[30:] + pads.get(s, []), rng), 5002.5 + (3 * s) % 5) for s in range(n)})
    assert f.ctx.stream_decoder_stats()[0] == 4222
    exp = f.fold(range(n))
    assert len(exp[0]) == 82 and (exp[1]["n_streams"][:7] == 70).all() and (exp[1]["n_streams"][7:29] == 1).all()
    same(f.merged(), exp)
    same(f.merged(cutoff=5003), f.fold(range(n), 5003))
    sel = list(range(3, 70, 2))
    same(f.merged(sel, 5004), f.fold(sel, 5004))
    f.close()


def test_three_streams_out_of_five_thousand(native):
    """Stream bits above the low nibbles: 5000 open streams, 0, 4097 and 4999 in use, selected as a list and by None."""
    rng = np.random.default_rng(92)
    f = Fleet(5000)
    addr = [0, 0xFFFFFF] + [0x200000 + 4099 * k for k in range(30)]
    use = [0, 4097, 4999]
    f.hear({s: (replies([a for a in addr if (a + s) % 5], rng), 7000.5 + k) for k, s in enumerate(use)})
    exp = f.fold(use)
    assert len(exp[0]) == len(addr)
    same(f.merged(use), exp)
    same(f.merged(), exp)
    same(f.merged([4097, 4999], 7002), f.fold([4097, 4999], 7002))
    assert len(f.merged([1, 2, 4096, 4098])[0]) == 0
    f.close()


def raw(c, sel, cutoff, rows, info, cap):
    n = ctypes.c_int32(-1)
    s = None if sel is None else np.array(sel, np.int32)
    rc = c.lib.adsb_stream_planes_merged(c._h, None if s is None else ctypes.c_void_p(s.ctypes.data), 0 if s is None else len(s), cutoff,
                                         None if rows is None else ctypes.c_void_p(rows.ctypes.data),
                                         None if info is None else ctypes.c_void_p(info.ctypes.data), cap, ctypes.byref(n))
    return rc, n.value


def test_refusals_cap_rules_and_untouched_state(native):
    rng = np.random.default_rng(93)
    for flags in (SD, T | DEC | AGES, T | DEC, 0):                                           # without either flag; a dense context
        c = N.Context(FS, THR, flags=flags)
        if flags & SD:
            c.open_streams(2)
        assert _code(c.merged_planes) == -EINVAL
        c.close()
    plain = N.Context(FS, THR, flags=SD)
    rx = frontend.Receivers(plain, 2)
    with pytest.raises(ValueError):
        rx.merged()
    with pytest.raises(ValueError):
        rx.table(0.0)
    plain.close()
    c, twin = N.Context(FS, THR, flags=SD | AGES), N.Context(FS, THR, flags=SD | AGES)
    assert _code(c.merged_planes) == -EINVAL                                                 # no streams yet
    b14 = np.array([ident(0x10 + k, rng) for k in range(12)], np.uint8)
    more = np.array(replies([0x10 + k for k in range(4, 16)], rng), np.uint8)
    iq, iq2 = stream(b14, FS)[0], stream(more, FS)[0]
    for x in (c, twin):
        x.open_streams(3)
        for s in range(3):
            x.set_stream_start(s, 500.5 + 100 * s)
        x.process_stream_batch(N.FMT_FC32, [0, 1, 2], [iq] * 3, end=True)
    assert c.merged_planes()[0].size == 12
    d0 = c.last_stream_decoded().tobytes()
    tk = c.submit_format_host(N.FMT_FC32, iq)
    assert _code(c.merged_planes) == -EBUSY
    c.wait(tk)
    last = c.last_result().tobytes()
    n32 = ctypes.c_int32(0)
    for sel in ([1, 1], [2, 0], [0, 3], [-1, 0]):
        assert raw(c, sel, 0, None, None, 0)[0] == -EINVAL, sel
    assert c.lib.adsb_stream_planes_merged(c._h, None, 0, 0, None, None, 0, None) == -EINVAL
    assert c.lib.adsb_stream_planes_merged(c._h, None, 0, 0, None, None, 4, ctypes.byref(n32)) == -EINVAL
    assert c.lib.adsb_stream_planes_merged(c._h, None, 0, 0, None, None, -1, ctypes.byref(n32)) == -EINVAL
    # cap rules
    rows, info = np.zeros(16, N.DECODED_DTYPE), np.zeros(16, N.MERGED_DTYPE)
    rows.view(np.uint8)[:] = 0x77
    info.view(np.uint8)[:] = 0x77
    assert raw(c, None, INT64_MIN, None, None, 0) == (-ENOSPC, 12)                           # the count query
    assert raw(c, None, INT64_MIN, rows, info, 11) == (-ENOSPC, 12)
    assert (rows.view(np.uint8) == 0x77).all() and (info.view(np.uint8) == 0x77).all()       # ... and nothing written
    assert raw(c, None, 601, None, None, 0) == (-ENOSPC, 12) and raw(c, None, 701, None, None, 0) == (0, 0)
    assert raw(c, [], INT64_MIN, None, None, 0) == (0, 0)
    assert raw(c, None, INT64_MIN, rows, info, 16) == (0, 12)
    assert (rows[12:].view(np.uint8) == 0x77).all() and (info[12:].view(np.uint8) == 0x77).all()
    full = c.merged_planes()
    assert full[0].tobytes() == rows[:12].tobytes() and full[1].tobytes() == info[:12].tobytes()
    assert (info["n_streams"][:12] == 3).all() and (info["last_seen"][:12] == 700).all() and (info["src_callsign"][:12] == 2).all()
    assert (info["src_altitude"][:12] == -1).all() and not info["pad"][:12].any()
    r2, i2 = np.zeros(12, N.DECODED_DTYPE), np.zeros(12, N.MERGED_DTYPE)
    assert raw(c, None, INT64_MIN, r2, None, 12) == (0, 12) and raw(c, None, INT64_MIN, None, i2, 12) == (0, 12)
    assert r2.tobytes() == full[0].tobytes() and i2.tobytes() == full[1].tobytes()
    # one stream alone is its own snapshot
    before = c.stream_planes(seen=True)
    for s in range(3):
        r, i = c.merged_planes([s])
        sr, ss, _ = c.stream_planes([s], seen=True)
        assert r.tobytes() == sr.tobytes() and np.array_equal(i["last_seen"], ss) and (i["n_streams"] == 1).all()
        for name in SRC:
            assert np.isin(i[name], (s, -1)).all()
    # nothing changed: the snapshot, the last results, the streams -- and what is decoded afterwards
    after = c.stream_planes(seen=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))               # (bytes: the rows hold NaNs)
    assert c.merged_planes()[1].tobytes() == full[1].tobytes() and c.merged_planes()[0].tobytes() == full[0].tobytes()
    assert c.last_stream_decoded().tobytes() == d0 and c.last_result().tobytes() == last
    assert [c.stream_state(s)[0] for s in range(3)] == [0, 0, 0]
    for x in (c, twin):
        x.process_stream_batch(N.FMT_FC32, [0, 2], [iq2] * 2, end=True)
    assert c.last_stream_decoded().tobytes() == twin.last_stream_decoded().tobytes()
    a, b = c.stream_planes(seen=True), twin.stream_planes(seen=True)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    same(c.merged_planes(), twin.merged_planes())
    c.close(); twin.close()


def test_selection_refusals_by_text_and_which_comes_first(native):
    """adsb_stream_planes_merged's refusals by adsb_last_error's text, and which of two mistakes at once is named: the missing
    n_out before everything about the streams, no streams before the selection, n_sel before the indices, the selection
    before -EBUSY."""
    vp = ctypes.c_void_p
    c = N.Context(FS, THR, flags=SD | AGES)
    n32 = ctypes.c_int32(-7)
    bad = np.array([2, 0], np.int32)

    def merged(k, n_out=n32):
        rc = c.lib.adsb_stream_planes_merged(c._h, vp(bad.ctypes.data), k, 0, None, None, 0, None if n_out is None else ctypes.byref(n_out))
        return rc, c.lib.adsb_last_error(c._h).decode()
    assert merged(-1, None) == (-EINVAL, "adsb_stream_planes_merged: n_out, or rows / info for cap > 0, missing")
    assert merged(-1) == (-EINVAL, "adsb_stream_planes_merged: no streams (adsb_streams_open first)")
    c.open_streams(3)
    iq = stream(np.array([ident(0x10 + k, np.random.default_rng(96)) for k in range(4)], np.uint8), FS)[0]
    tk = c.submit_format_host(N.FMT_FC32, iq)                                   # busy: a bad selection is still named first
    assert merged(-1) == (-EINVAL, "adsb_stream_planes_merged: n_sel < 0")
    assert merged(2) == (-EINVAL, "adsb_stream_planes_merged: stream indices have to be in range and strictly ascending")
    assert merged(0)[0] == merged(1)[0] == -EBUSY
    c.wait(tk)
    assert merged(1)[0] == 0 and n32.value == 0                                 # stream 2 alone: nothing heard yet
    c.close()


def test_merged_around_an_expiry(native):
    rng = np.random.default_rng(94)
    f = Fleet(3)
    addr = [0x330000 + 7 * k for k in range(20)]
    f.hear({0: (replies(addr, rng), 1000.5), 1: (replies(addr[5:], rng), 1100.5)})
    f.hear({2: (replies(addr[:12], rng), 1200.5)})
    same(f.merged(), f.fold(range(3)))
    hidden = f.merged(cutoff=1100)
    same(hidden, f.fold(range(3), 1100))
    n = f.mod.m[0].sweep(1100) + f.mod.m[1].sweep(1100) + f.mod.m[2].sweep(1100)
    assert n == 20 and f.rx.expire(1100) == n
    same(f.merged(), hidden)                                             # what the cutoff hid is what the expiry removed
    same(f.merged(), f.fold(range(3)))
    f.check()
    lines = f.rx.table(1300.0)
    assert lines == N.plane_table(hidden[0], 1300.0) and len(lines) == 20
    f.close()


def test_buffers_across_close_and_open(native):
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    rng = np.random.default_rng(95)
    iq = stream(np.array([ident(0x100 + k, rng) for k in range(20)], np.uint8), FS)[0]
    c = N.Context(FS, THR, flags=SD | AGES)
    left, first = [], None
    for rep in range(6):
        c.open_streams(4)
        assert c.merged_planes()[0].size == 0                             # a new fleet: nothing of the last one
        for s in range(4):
            c.set_stream_start(s, 100.5 + s)
        c.process_stream_batch(N.FMT_FC32, [0, 1, 2, 3], [iq] * 4, end=True)
        rows, info = c.merged_planes()
        assert len(rows) == 20 and (info["n_streams"] == 4).all() and (info["last_seen"] == 103).all()
        if first is None:
            first = (rows.tobytes(), info.tobytes())
        assert (rows.tobytes(), info.tobytes()) == first
        c.close_streams()
        assert _code(c.merged_planes) == -EINVAL
        left.append(free())
    assert left[2] - left[5] < (16 << 20), [(x - left[0]) >> 20 for x in left]
    c.close()
