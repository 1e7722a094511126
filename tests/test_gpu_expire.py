"""Plane ages on the MI355X (ADSB_FLAG_PLANE_AGES: adsb_planes_seen / adsb_stream_planes_seen, adsb_planes_expire /
adsb_stream_planes_expire behind the host code of adsb_hip.hip): tests/golden/g_expire.npz -- the reference decoder with
`del plane_dict[key]` between PDUs -- through adsb_decode_pdus and through both stream-batch entry points, the dense scan's
edge addresses, the 256-slot store, the refusals and the untouched-state guarantees, the buffers' lifecycle.  The CPU half
(emulator, the golden itself, the model) is tests/test_expire.py.  Nothing here reads the reference tree."""
import ctypes

import numpy as np
import pytest

import decode_streams as S
import test_decode as TD
import test_planes as TP
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from test_expire import (CONFIGS, GARBAGE, INT64_MIN, FleetModel, Model, ap4, cluster_addresses, df11, expire_lib, gold_dict, ident,
                         run_golden, sequences, AgedFleet)
from test_gpu_decode import THR, stream
from test_gpu_stream_decode import FS

pytestmark = pytest.mark.gpu

T, F, DEC, SD, AGES = N.FLAG_AIRCRAFT_TABLE, N.FLAG_FEC_CONSERVATIVE, N.FLAG_DECODE, N.FLAG_STREAM_DECODE, N.FLAG_PLANE_AGES
ENOSPC, EINVAL, EBUSY = 28, 22, 16
CHUNK, TOP = TP.CHUNK, TP.TOP


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


@pytest.fixture(scope="module")
def ge():
    return np.load(TD.GOLD.replace("g_decode.npz", "g_expire.npz"))


def _code(fn, *a, **k):
    with pytest.raises(N.AdsbError) as e:
        fn(*a, **k)
    return e.value.code


def dense_ctx(filt, corr, extra=AGES):
    c = N.Context(2e6, THR, flags=T | DEC | extra | (F if corr == "Conservative" else 0))
    c.set_decoder(filt, 0.0)
    return c


def check_dense(c, mod):
    rows, seen = c.planes(seen=True)
    erows, eseen = mod.snapshot()
    TP.rows_equal(rows, erows)
    assert np.array_equal(seen, eseen)
    assert c.planes().tobytes() == rows.tobytes()            # the plain snapshot: the same rows


# ---- one decoder -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_decode_pdus_expire_and_seen_equal_the_golden(native, ge, tag, filt, corr):
    c = dense_ctx(filt, corr)

    class Dec:
        call = staticmethod(c.decode_pdus)
        expire = staticmethod(c.expire_planes)

        @staticmethod
        def snapshot():
            rows, seen = c.planes(seen=True)
            assert c.planes().tobytes() == rows.tobytes()
            return rows, seen

    def make():
        c.reset()
        return Dec
    for how in ("points", "random"):
        run_golden(ge, tag, make, how)
    c.close()


def test_dense_edge_addresses(native):
    """Addresses 0, 1, 2047, 2048, 0xFFFFFE, 0xFFFFFF, stale / fresh pairs of one 16-byte load, a chunk that loses every plane,
    300 others; what is expired is unknown to an address/parity reply and starts over when heard again; an announced address
    without a plane is left alone; after reset() nothing is left to expire."""
    rng = np.random.default_rng(81)
    edge = [0, 1, CHUNK - 1, CHUNK, 0xFFFFFE, 0xFFFFFF]
    pairs = [0x300010, 0x300011, 0x300020, 0x300021]
    full = list(range(5 * CHUNK, 5 * CHUNK + 40))
    others = [0x400000 + 523 * k for k in range(300)]
    old = edge[::2] + [pairs[0], pairs[3]] + full + others[::2]
    new = edge[1::2] + [pairs[1], pairs[2]] + others[1::2]
    c, mod = dense_ctx("All Messages", "None"), Model("All Messages", "None")
    b = [ident(a, rng) for a in old + new]
    t = [5000.5 + 0.01 * k for k in range(len(old))] + [5100.5 + 0.01 * k for k in range(len(new))]
    TP.rows_equal(c.decode_pdus(b, t), mod.rows(b, t))
    check_dense(c, mod)
    assert c.expire_planes(5050) == mod.sweep(5050) == len(old)
    check_dense(c, mod)
    assert c.expire_planes(5050) == 0
    b = [ap4(a, rng) for a in old + new]
    t = [5200.5 + 0.001 * k for k in range(len(b))]
    got = c.decode_pdus(b, t)
    TP.rows_equal(got, mod.rows(b, t))
    assert not (got["present"][:len(old)] & N.DEC_HAS_PLANE).any() and (got["present"][len(old):] & N.DEC_HAS_PLANE).all()
    b, t = [ident(a, rng) for a in old[:9]] + [ap4(a, rng) for a in old[:9]], [5300.5] * 18
    got = c.decode_pdus(b, t)
    TP.rows_equal(got, mod.rows(b, t))
    assert got["num_msgs"].tolist() == [1] * 9 + [2] * 9
    check_dense(c, mod)
    c.reset()
    assert c.expire_planes(1 << 62) == 0 and len(c.planes(seen=True)[0]) == 0
    c.close()
    c = dense_ctx("Extended Squitter Only", "None")
    got = c.decode_pdus([df11(0x123456), ident(0x123457, rng), ident(0x123458, rng)], [10.5, 11.5, 99.5])
    assert (got["present"] & N.DEC_HAS_PLANE).tolist() == [0, 1, 1]
    assert c.expire_planes(50) == 1
    rows, seen = c.planes(seen=True)
    assert rows["icao"].tolist() == [0x123458] and seen.tolist() == [99]
    c.close()


def test_dense_refusals_and_untouched_state(native):
    """-EINVAL without the flag (and the flag alone is no context); -EBUSY while a ticket is pending; an expiry and a snapshot
    leave adsb_last_result / adsb_last_decoded and the framer state as they were; a no-op expiry changes no later byte."""
    rng = np.random.default_rng(82)
    n64, n32 = ctypes.c_int64(0), ctypes.c_int32(0)
    for flags in (AGES, AGES | T, AGES | N.FLAG_CONFIDENCE):
        with pytest.raises(N.AdsbError) as e:
            N.Context(FS, THR, flags=flags)
        assert e.value.code == -EINVAL
    for flags in (0, T | DEC, SD):
        c = N.Context(FS, THR, flags=flags)
        assert _code(c.expire_planes, 0) == -EINVAL and _code(c.planes, seen=True) == -EINVAL
        assert _code(c.expire_stream_planes, []) == -EINVAL
        c.close()
    addr = [0x111111, 0x222222, 0x333333]
    b14, _ = S.mixed(rng, n=90, addresses=addr)
    iq, _ = stream(b14, FS)
    c, plain = N.Context(FS, THR, flags=T | DEC | AGES), N.Context(FS, THR, flags=T | DEC | AGES)
    for x in (c, plain):
        x.set_decoder("All Messages", 1000.25)
    assert c.lib.adsb_planes_seen(c._h, None, None, 4, ctypes.byref(n32)) == -EINVAL
    assert c.lib.adsb_planes_seen(c._h, None, None, 0, None) == -EINVAL
    assert _code(c.expire_stream_planes, []) == -EINVAL                     # not a fleet
    tk = c.submit_format_host(N.FMT_FC32, iq)
    assert _code(c.expire_planes, 0) == -EBUSY and _code(c.planes, seen=True) == -EBUSY
    r0 = c.wait(tk)
    r1 = plain.process_format(N.FMT_FC32, iq)
    assert r0.tobytes() == r1.tobytes()
    d0, state = c.last_decoded().tobytes(), c.framer_state()
    rows, seen = c.planes(seen=True)
    k = len(rows)
    assert 1 <= k <= 3 and (seen == 1000).all()
    assert c.lib.adsb_planes_expire(c._h, INT64_MIN, None) == 0 and c.expire_planes(1000) == 0         # == cutoff stays
    assert c.last_decoded().tobytes() == d0 == plain.last_decoded().tobytes() and c.framer_state() == state
    assert c.last_result().tobytes() == r0.tobytes()
    only_seen = np.zeros(k, np.int64)
    assert c.lib.adsb_planes_seen(c._h, None, ctypes.c_void_p(only_seen.ctypes.data), k, ctypes.byref(n32)) == 0 and n32.value == k
    assert np.array_equal(only_seen, seen)
    assert c.lib.adsb_planes_seen(c._h, None, ctypes.c_void_p(only_seen.ctypes.data), k - 1, ctypes.byref(n32)) == -ENOSPC and n32.value == k
    b2, t2 = S.mixed(rng, n=200, addresses=addr + [0x444444], t0=1003.5)
    S.assert_rows_equal(c.decode_pdus(b2, t2), plain.decode_pdus(b2, t2))
    a, p = c.planes(seen=True), plain.planes(seen=True)
    assert a[0].tobytes() == p[0].tobytes() and np.array_equal(a[1], p[1])
    c.close(); plain.close()


def test_flag_off_allocates_nothing_and_every_buffer_is_released(native):
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    rng = np.random.default_rng(83)
    b = [ident(0x100 + k, rng) for k in range(50)]
    t = [100.5 + k for k in range(50)]

    def dense(extra):
        c = dense_ctx("All Messages", "None", extra)
        c.decode_pdus(b, t)
        held = free()
        if extra:
            assert c.expire_planes(120) == 20 and len(c.planes(seen=True)[0]) == 30
        c.close()
        return held

    def fleet():
        c = N.Context(FS, THR, flags=SD | AGES)
        c.open_streams(4)
        c.stream_decoder_reserve(256)
        iq = stream(np.array(b[:20], np.uint8), FS)[0]
        c.process_stream_batch(N.FMT_FC32, [0, 1, 2, 3], [iq] * 4, end=True)
        assert c.expire_stream_planes([1 << 40] * 4) == 80 and c.stream_decoder_stats()[0] == 0
        c.close()                                     # with streams open: adsb_destroy releases them
    dense(AGES); dense(0)
    base = free()
    with_flag, without = base - dense(AGES), base - dense(0)
    assert (120 << 20) < with_flag - without < (140 << 20), (with_flag >> 20, without >> 20)      # 2^24 int64, and the flag alone
    left = []
    for rep in range(8):
        dense(AGES)
        fleet()
        left.append(free())
    assert left[3] - left[7] < (16 << 20), [(x - left[0]) >> 20 for x in left]


# ---- the fleet -----------------------------------------------------------------------------------------------------------------
def pdu_iq(b14):
    """One reply as a stream chunk of its own (tests/test_gpu_decode.py stream: the burst 400 samples in)."""
    return stream(np.asarray(b14, np.uint8).reshape(1, 14), FS)[0]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("tag,filt,corr", CONFIGS[:2])
def test_stream_batch_expire_and_seen_equal_the_golden(native, ge, tag, filt, corr, device):
    """The golden's four sequences as four receivers of one 256-slot store.  Every PDU is a chunk of its own that ends its
    stream (an END item leaves the decoder alone), so that the stream's start can put the PDU's clock where the golden has it:
    call k holds PDU k of every sequence that still has one, a sequence's deletion points in front of its PDU as
    adsb_stream_planes_expire with that stream selected."""
    import torch
    seqs = sequences(ge)
    c = N.Context(FS, THR, flags=SD | AGES | (F if corr == "Conservative" else 0))
    c.open_streams(len(seqs))
    c.set_streams_decoder(filt)
    c.stream_decoder_reserve(256)
    got = np.zeros(len(ge["bits"]), dtype=N.DECODED_DTYPE)
    keep = []

    def sweep(s, p, cutoff):
        rows, seen, first = c.stream_planes([s], seen=True)
        e, eseen = gold_dict(ge, tag, "b", p)
        TP.check_against_golden(rows, e, (tag, p))
        assert np.array_equal(seen, eseen) and first.tolist() == [0, len(rows)]
        before = c.stream_planes()[0]
        assert c.expire_stream_planes([cutoff], [s]) == int(ge["del_removed_" + tag][p])
        after, first = c.stream_planes()
        assert c.stream_decoder_stats()[0] == len(after) == len(before) - int(ge["del_removed_" + tag][p])
    for k in range(max(sl.stop - sl.start for sl, _ in seqs) + 1):
        ids, chunks, where = [], [], []
        for s, (sl, pts) in enumerate(seqs):
            for p, at, cutoff in pts:
                if at == k:
                    sweep(s, p, cutoff)
            if sl.start + k < sl.stop:
                i = sl.start + k
                c.set_stream_start(s, float(ge["ts"][i]) - 400 / FS)
                ids.append(s); chunks.append(pdu_iq(ge["bits"][i])); where.append(i)
        if not ids:
            continue
        if device:
            dev = [torch.from_numpy(x.view(np.float32).copy()).cuda() for x in chunks]
            keep.append(dev)
            recs, first = c.process_stream_batch_device(N.FMT_FC32, ids, [d.data_ptr() for d in dev], [len(x) for x in chunks], end=True)
        else:
            recs, first = c.process_stream_batch(N.FMT_FC32, ids, chunks, end=True)
        rows = c.last_stream_decoded()
        assert first.tolist() == list(range(len(ids) + 1)), (k, first)          # one record per chunk
        assert ((recs["flags"] & N.BURST_DEMOD) != 0).all()
        for j, (s, i) in enumerate(zip(ids, where)):
            ts = (float(ge["ts"][i]) - 400 / FS) + int(recs["offset"][j]) / FS
            assert int(ts) == int(ge["ts"][i]), (i, ts)                          # the decoder's clock is the golden's
        got[where] = rows
    TD.check_rows(got, ge, tag)
    rows, seen, first = c.stream_planes(seen=True)
    for s in range(len(seqs)):
        e, eseen = gold_dict(ge, tag, "f", s)
        TP.check_against_golden(rows[first[s]:first[s + 1]], e, (tag, "end", s))
        assert np.array_equal(seen[first[s]:first[s + 1]], eseen)
    assert c.stream_decoder_stats()[:2] == (len(rows), 256)
    c.close()


class GpuFleet:
    """Receivers that hear whole chunks of replies at a start time of our choosing; the model gets the records' timestamps."""

    def __init__(self, n, filt="All Messages", corr="None", slots=256):
        self.fe = frontend.FrontEnd(FS, THR, flags=SD | AGES | (F if corr == "Conservative" else 0))
        self.rx = self.fe.receivers(n, fmt=N.FMT_FC32, msg_filter=filt, ages=True)
        self.ctx = self.fe.ctx
        self.ctx.stream_decoder_reserve(slots)
        self.mod = FleetModel(n, filt, corr)

    def hear(self, chunks):
        """{stream: (replies, start)}: one call, every stream ended -> {stream: rows}"""
        ids = sorted(chunks)
        for s in ids:
            self.ctx.set_stream_start(s, chunks[s][1])
        recs = self.rx.push([stream(np.array(chunks[s][0], np.uint8), FS)[0] for s in ids], ids=ids)
        rows = self.rx.rows
        fin, frows = self.rx.finish(ids), self.rx.rows
        out = {}
        for s, r, d, r2, d2 in zip(ids, recs, rows, fin, frows):
            r, d = np.concatenate([r, r2]), np.concatenate([d, d2])
            assert len(r) == len(chunks[s][0]) and ((r["flags"] & N.BURST_DEMOD) != 0).all()
            exp = self.mod.m[s].rows(r["bits"], [chunks[s][1] + int(o) / FS for o in r["offset"]])
            TP.rows_equal(d, exp)
            out[s] = d
        return out

    def check(self):
        got = self.rx.planes(seen=True)
        for (rows, seen), m in zip(got, self.mod.m):
            erows, eseen = m.snapshot()
            TP.rows_equal(rows, erows)
            assert np.array_equal(seen, eseen)
        plain = self.rx.planes()
        assert [x.tobytes() for x in plain] == [r.tobytes() for r, _ in got]
        assert self.ctx.stream_decoder_stats()[0] == self.mod.planes()

    def close(self):
        self.rx.close()
        self.ctx.close()


def test_store_of_256_slots(native):
    """Three receivers, 95 planes in a store reserved at its minimum: a probe cluster that wraps from slot 255 to slot 0 loses
    its middle and every survivor is still found; the same addresses in two streams with different cutoffs while the third is
    not selected; a reset stream's stale slots and an expiry in one pass; expiry, growth, expiry."""
    rng = np.random.default_rng(84)
    sim = expire_lib()
    hasher = AgedFleet(sim, 1, "All Messages", "None")
    clus = cluster_addresses(hasher, 30)                 # home slots 236 .. 255 of a 256-slot store: they wrap
    hasher.close()
    shared = [0x700000 + 11 * k for k in range(25)]
    f = GpuFleet(3)
    idents = lambda addrs: [ident(a, rng) for a in addrs]                      # noqa: E731
    aps = lambda addrs: [ap4(a, rng) for a in addrs]                           # noqa: E731
    f.hear({0: (idents(clus[10:20]), 910.5)})
    f.hear({0: (idents(clus[:10] + clus[20:] + shared), 1000.5), 1: (idents(shared), 1000.5), 2: (idents(shared[:15]), 1000.5)})
    assert f.ctx.stream_decoder_stats() == (95, 256, 0)
    f.check()
    assert f.rx.expire(950) == f.mod.m[0].sweep(950) == 10
    f.check()
    d = f.hear({0: (aps(clus), 1001.5)})[0]
    assert ((d["present"] & N.DEC_HAS_PLANE) != 0).tolist() == [True] * 10 + [False] * 10 + [True] * 10
    f.hear({0: (idents(shared[:5]), 1100.5), 1: (idents(shared[:12]), 1100.5)})
    n = f.mod.m[0].sweep(1001) + f.mod.m[1].sweep(1100)
    assert n == 20 + 13 and f.rx.expire([1001, 1100], ids=[0, 1]) == n         # stream 0 keeps what it heard at 1001 and 1100
    f.check()
    assert len(f.rx.planes([2])[0]) == 15
    f.ctx.reset_stream(2)
    f.mod.reset(2)
    n = f.mod.m[1].sweep(1 << 40)
    assert n == 12 and f.ctx.expire_stream_planes([1 << 40], [1]) == n
    f.check()
    d = f.hear({s: (aps(shared), 1200.5) for s in range(3)})
    assert [int(((d[s]["present"] & N.DEC_HAS_PLANE) != 0).sum()) for s in range(3)] == [5, 0, 0]
    # growth then expiry then growth: last_seen survives every rehash
    more = [0x900000 + 13 * k for k in range(300)]
    f.hear({1: (idents(more[:150]), 2000.5), 2: (idents(more), 2100.5)})
    planes, cap, grows = f.ctx.stream_decoder_stats()
    assert planes == f.mod.planes() and cap >= 1024 and grows >= 1
    f.check()
    n = f.mod.m[0].sweep(2050) + f.mod.m[1].sweep(2050) + f.mod.m[2].sweep(2050)
    assert n == 25 + 150 and f.rx.expire(2050) == n
    f.check()
    f.hear({0: (idents(more), 2200.5), 1: (idents(more + shared), 2200.5)})
    assert f.ctx.stream_decoder_stats()[1] > cap
    f.check()
    with pytest.raises(ValueError):
        f.rx.expire([1, 2])
    with pytest.raises(ValueError):
        f.ctx.expire_stream_planes([1, 2], [1, 0])
    f.close()


def test_fleet_refusals_and_untouched_state(native):
    rng = np.random.default_rng(85)
    n64 = ctypes.c_int64(0)
    c = N.Context(FS, THR, flags=SD | AGES)
    assert _code(c.expire_stream_planes, []) == -EINVAL and _code(c.stream_planes, seen=True) == -EINVAL      # no streams yet
    assert _code(c.expire_planes, 0) == -EINVAL                                                               # not one decoder
    c.open_streams(3)
    b14 = np.array([ident(0x10 + k, rng) for k in range(12)], np.uint8)
    iq = stream(b14, FS)[0]
    for s in range(3):
        c.set_stream_start(s, 500.5 + 100 * s)
    recs, first = c.process_stream_batch(N.FMT_FC32, [0, 1, 2], [iq] * 3, end=True)
    d0 = c.last_stream_decoded().tobytes()
    tk = c.submit_format_host(N.FMT_FC32, iq)
    assert _code(c.expire_stream_planes, [0, 0, 0]) == -EBUSY and _code(c.stream_planes, seen=True) == -EBUSY
    c.wait(tk)
    last = c.last_result().tobytes()
    cut = np.array([0, 0], np.int64)
    for sel in ([1, 1], [2, 0], [0, 3], [-1, 0]):
        s = np.array(sel, np.int32)
        assert c.lib.adsb_stream_planes_expire(c._h, ctypes.c_void_p(s.ctypes.data), 2, ctypes.c_void_p(cut.ctypes.data), ctypes.byref(n64)) == -EINVAL
    assert c.lib.adsb_stream_planes_expire(c._h, None, 0, None, ctypes.byref(n64)) == -EINVAL
    rows, seen, f1 = c.stream_planes(seen=True)
    assert list(f1) == [0, 12, 24, 36] and seen.tolist() == [500] * 12 + [600] * 12 + [700] * 12
    assert c.expire_stream_planes([INT64_MIN] * 3) == 0 and c.expire_stream_planes([500, 600, 700]) == 0
    assert c.lib.adsb_stream_planes_expire(c._h, None, 0, ctypes.c_void_p(np.array([0, 0, 0], np.int64).ctypes.data), None) == 0
    r2, s2, f2 = c.stream_planes(seen=True)
    assert r2.tobytes() == rows.tobytes() and np.array_equal(s2, seen)
    assert c.last_stream_decoded().tobytes() == d0 and c.last_result().tobytes() == last
    assert [c.stream_state(s)[0] for s in range(3)] == [0, 0, 0]
    assert c.expire_stream_planes([601], [1]) == 12                           # its own clock; the others lose nothing
    rows, seen, f1 = c.stream_planes(seen=True)
    assert list(f1) == [0, 12, 12, 24] and c.stream_decoder_stats()[0] == 24
    only = c.stream_planes([2], seen=True)
    assert only[1].tolist() == [700] * 12 and only[0].tobytes() == rows[12:].tobytes()
    c.close()
    plain = N.Context(FS, THR, flags=SD)
    with pytest.raises(ValueError):
        frontend.Receivers(plain, 2, ages=True)
    rx = frontend.Receivers(plain, 2)
    with pytest.raises(ValueError):
        rx.expire(0)
    with pytest.raises(ValueError):
        rx.planes(seen=True)
    plain.close()


def test_fleet_selection_refusals_by_text_and_snapshots_in_parts(native):
    """The stream selection of adsb_stream_planes / _seen / _expire, refusal by refusal, by adsb_last_error's text, and which of
    two mistakes at once is named: no streams before the selection, n_sel before the indices (the expiry: missing cutoffs
    with it), the selection before -EBUSY.  Then the snapshot with ages in parts: an empty selection zeroes its first[],
    -ENOSPC leaves the count, rows alone and last_seen alone are those of the whole call."""
    vp, ref = ctypes.c_void_p, ctypes.byref
    rng = np.random.default_rng(86)
    c = N.Context(FS, THR, flags=SD | AGES)
    lib, h = c.lib, c._h
    n32, n64 = ctypes.c_int32(-7), ctypes.c_int64(-7)
    bad, cut = np.array([2, 0], np.int32), np.zeros(3, np.int64)
    badp, cutp = vp(bad.ctypes.data), vp(cut.ctypes.data)

    def planes(sp, k):
        return lib.adsb_stream_planes(h, sp, k, None, 0, None, ref(n32)), lib.adsb_last_error(h).decode()

    def seen(sp, k):
        return lib.adsb_stream_planes_seen(h, sp, k, None, None, 0, None, ref(n32)), lib.adsb_last_error(h).decode()

    def expire(sp, k, cp):
        return lib.adsb_stream_planes_expire(h, sp, k, cp, ref(n64)), lib.adsb_last_error(h).decode()
    closed = "%s: no streams (adsb_streams_open first)"
    assert planes(badp, -1) == seen(badp, -1) == (-EINVAL, closed % "adsb_stream_planes")
    assert expire(badp, -1, None) == (-EINVAL, closed % "adsb_stream_planes_expire")
    c.open_streams(3)
    iq = stream(np.array([ident(0x10 + k, rng) for k in range(12)], np.uint8), FS)[0]
    tk = c.submit_format_host(N.FMT_FC32, iq)                                   # busy: a bad selection is still named first
    order = "%s: stream indices have to be in range and strictly ascending"
    assert planes(badp, -1) == seen(badp, -1) == (-EINVAL, "adsb_stream_planes: n_sel < 0")
    assert planes(badp, 2) == seen(badp, 2) == (-EINVAL, order % "adsb_stream_planes")
    missing = (-EINVAL, "adsb_stream_planes_expire: n_sel < 0, or cutoffs missing")
    assert expire(badp, -1, cutp) == missing and expire(badp, 2, None) == missing and expire(None, 0, None) == missing
    assert expire(badp, 2, cutp) == (-EINVAL, order % "adsb_stream_planes_expire")
    assert planes(None, 0)[0] == seen(None, 0)[0] == expire(None, 0, cutp)[0] == expire(badp, 0, None)[0] == -EBUSY
    c.wait(tk)
    first = np.full(4, 0x55555555, np.int32)
    sel = np.array([0, 2], np.int32)
    assert lib.adsb_stream_planes_seen(h, vp(sel.ctypes.data), 2, None, None, 0, vp(first.ctypes.data), ref(n32)) == 0
    assert n32.value == 0 and first.tolist() == [0, 0, 0, 0x55555555]
    for s in range(3):
        c.set_stream_start(s, 500.5 + 100 * s)
    c.process_stream_batch(N.FMT_FC32, [0, 1, 2], [iq] * 3, end=True)
    rows, ages, f0 = c.stream_planes(seen=True)
    assert len(rows) == 36 and list(f0) == [0, 12, 24, 36]
    r, a = np.zeros(36, N.DECODED_DTYPE), np.zeros(36, np.int64)
    r.view(np.uint8)[:] = 0x77
    assert lib.adsb_stream_planes_seen(h, None, 0, vp(r.ctypes.data), vp(a.ctypes.data), 35, vp(first.ctypes.data), ref(n32)) == -ENOSPC
    assert lib.adsb_last_error(h).decode() == "adsb_stream_planes: cap is smaller than the number of planes (*n_out)"
    assert n32.value == 36 and (r.view(np.uint8) == 0x77).all() and not a.any() and first.tolist() == [0, 0, 0, 0x55555555]
    assert lib.adsb_stream_planes_seen(h, None, 0, vp(r.ctypes.data), None, 36, vp(first.ctypes.data), ref(n32)) == 0
    assert r.tobytes() == rows.tobytes() and first.tolist() == [0, 12, 24, 36] and not a.any()
    assert lib.adsb_stream_planes_seen(h, vp(sel.ctypes.data), 2, None, vp(a.ctypes.data), 36, None, ref(n32)) == 0
    assert n32.value == 24 and a[:24].tolist() == ages[:12].tolist() + ages[24:].tolist() and not a[24:].any()
    c.close()


def test_decoder_block_with_a_plane_timeout(native, ge):
    """blocks.decoder(plane_timeout=60) on the device: the model with the sweep last_seen < int(timestamp) - 60 in front of
    every PDU; plane_dict carries last_seen; the default block sweeps nothing."""
    from gr_adsb_amd import blocks
    sl = TD.seq_slices(ge["seq"])[0]
    bits, ts = ge["bits"][sl], ge["ts"][sl]
    pdus = [({"timestamp": float(t), "snr": 1.0}, np.unpackbits(b)) for b, t in zip(bits, ts)]
    blk, plain, mod = blocks.decoder("All Messages", "Conservative", plane_timeout=60), blocks.decoder("All Messages", "Conservative"), \
        Model("All Messages", "Conservative")
    removed = 0
    for k, p in enumerate(pdus):
        removed += mod.sweep(int(ts[k]) - 60)
        mod.row(bits[k], ts[k])
        blk.decode_packet(p)
    plain.decode_pdus(pdus)
    assert removed >= 5
    erows, eseen = mod.snapshot()
    pd = blk.plane_dict
    assert list(pd) == ["{:06x}".format(int(a)) for a in erows["icao"]]
    assert [d["last_seen"] for d in pd.values()] == eseen.tolist() and [d["num_msgs"] for d in pd.values()] == erows["num_msgs"].tolist()
    assert len(plain.plane_dict) > len(pd) and all("last_seen" not in d for d in plain.plane_dict.values())
    blk.stop(); plain.stop()
