"""adsb_process_batch* on the MI355X: a batch of independent streams in one device pass (k_batch + k_batch_pack) against the
reference's single-call vectors, against a loop of adsb_process_format_device on a second context, and against the C oracle.
Every comparison is byte for byte.  `last_batch_fallbacks` is asserted in every test: outside the fallback test it must
equal the number of items that are longer than ADSB_BATCH_ITEM_MAX or are the vector Qpaths_4msps (whose preamble train
overflows the first list capacity), so that the batch kernel itself is what the comparisons exercise.
The CPU half (emulator) is tests/test_batch.py."""
import ctypes

import numpy as np
import pytest

import helpers
from gr_adsb_amd import _native as N
from gr_adsb_amd import modulator as M

pytestmark = pytest.mark.gpu

ENOSPC, EBUSY, EINVAL = 28, 16, 22
FMT_SCALE = {N.FMT_SC16: 2.0 / 32767.0, N.FMT_SC8: 2.0 / 127.0, N.FMT_CU8: 2.0 / 255.0}
GARBAGE = 0x41           # 0x41414141 = 12.08f, 16705 as int16, 65 as int8: "high" in every format -- a leak from a neighbour shows


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


def make_ctx(fs, thr=0.01, flags=0, scales=FMT_SCALE):
    c = N.Context(fs, thr, flags=flags)
    for f, s in (scales or {}).items():
        c.set_format_scale(f, s)
    return c


def to_format(fmt, iq):
    if fmt == N.FMT_FC32:
        return np.ascontiguousarray(iq, dtype=np.complex64)
    if fmt == N.FMT_MAG2:
        return M.mag2(iq)
    if fmt == N.FMT_SC16:
        return M.quantize_iq16(iq)
    return M.quantize_iq8(iq, offset_binary=(fmt == N.FMT_CU8))


class DeviceItems:
    """Host arrays (format layout) placed in ONE device allocation: back to back (each start rounded up to 16 bytes) or
    scattered (random gaps); the allocation is filled with GARBAGE first."""

    def __init__(self, ctx, fmt, arrays, scattered=False, seed=0):
        self.ctx = ctx
        rng = np.random.default_rng(seed)
        per = N.FMT_LAYOUT[fmt][1]
        offs, pos = [], 0
        for a in arrays:
            if scattered:
                pos += 16 * int(rng.integers(0, 40))
            offs.append(pos)
            pos += (a.nbytes + 15) // 16 * 16
        total = pos + 256
        host = np.full(total, GARBAGE, dtype=np.uint8)
        for a, o in zip(arrays, offs):
            host[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.base = ctx.device_alloc(total)
        ctx.device_upload(self.base, host)
        self.ptrs = [self.base + o for o in offs]
        self.ns = [len(a) // per for a in arrays]

    def free(self):
        self.ctx.device_free(self.base)


def loop(ctx, fmt, items, thrs, offs=None):
    """the same items one call each: what the batch must equal"""
    out, first = [], [0]
    for i, (p, n) in enumerate(zip(items.ptrs, items.ns)):
        ctx.set_threshold(thrs[i])
        r = ctx.process_format_device(fmt, p, n, 0 if offs is None else offs[i])
        out.append(r)
        first.append(first[-1] + len(r))
    return (np.concatenate(out) if out else np.zeros(0, dtype=N.BURST_DTYPE)), np.array(first, dtype=np.int32)


def expected_fallbacks(ns, names=None):
    return sum(1 for i, n in enumerate(ns) if n > N.BATCH_ITEM_MAX or (names is not None and names[i] == "Qpaths_4msps"))


# ---- 1. reference-pinned -------------------------------------------------------------------------------------------------
def _goldens(sps):
    names = (helpers.golden_names() + helpers.large_golden_names() + helpers.pathological_names() +
             helpers.path_golden_names())
    return [g for g in (helpers.Golden(n) for n in names) if g.sps == sps]


def _check_goldens(ctx, fmt, gs, arrays):
    items = DeviceItems(ctx, fmt, arrays)
    offs = [7000 * i for i in range(len(gs))]
    recs, first = ctx.process_batch_device(fmt, items.ptrs, items.ns, [g.thr for g in gs], offs)
    assert ctx.last_batch_fallbacks == expected_fallbacks(items.ns, [g.name for g in gs])
    assert first[0] == 0 and first[-1] == len(recs) and len(first) == len(gs) + 1
    for i, g in enumerate(gs):
        r = recs[first[i]:first[i + 1]].copy()
        r["offset"] -= offs[i]
        helpers.assert_recs_match_golden(r, g)
    items.free()
    return len(recs)


@pytest.mark.parametrize("sps", [2, 4, 8, 20])
def test_every_golden_of_a_rate_in_one_call(native, sps):
    gs = _goldens(sps)
    if sps == 2:
        assert len(gs) == 24
    ctx = make_ctx(sps * 1e6)
    assert _check_goldens(ctx, N.FMT_MAG2, gs, [np.asarray(g.x, dtype=np.float32) for g in gs]) > 100
    ci = [g for g in gs if g.iq is not None]
    assert len(ci) >= 2
    assert _check_goldens(ctx, N.FMT_FC32, ci, [g.iq for g in ci]) > 100
    for g in gs:
        if g.iq8 is not None:                               # the L* vectors, each with its own scale
            same = [h for h in gs if h.iq8 is not None and h.scale == g.scale]
            ctx.set_format_scale(N.FMT_SC8, float(g.scale))
            assert _check_goldens(ctx, N.FMT_SC8, same, [h.iq8 for h in same]) > 100
    ctx.close()


def test_run_time_stride_goldens_in_one_call(native):
    gs = [helpers.Golden("R12msps"), helpers.Golden("Qpaths_12msps")]
    ctx = make_ctx(12e6)
    assert _check_goldens(ctx, N.FMT_MAG2, gs, [np.asarray(g.x, dtype=np.float32) for g in gs]) > 10
    ctx.close()


# ---- 2. against the library itself -------------------------------------------------------------------------------------
_pools = {}


def pool(fs):
    if fs not in _pools:
        _pools[fs] = M.synth_iq(1 << 21, fs, 2000, seed=int(fs // 1e6) + 40)
    return _pools[fs]


def random_items(fs, fmt, k, rng, max_log2=18):
    """k items cut out of the pool: lengths 0 .. 2^max_log2, the edge lengths forced in, a few long ones"""
    iq = pool(fs)
    forced = [0, 1, 15, 16, 17, 1023, 1024, 1025, 1 << max_log2]
    lens = []
    for i in range(k):
        if k >= 63 and i < len(forced):
            lens.append(forced[i])
        elif rng.random() < 0.05 or k <= 2:
            lens.append(int(2 ** rng.uniform(14, max_log2)))
        else:
            lens.append(int(2 ** rng.uniform(0, 14)))
    order = rng.permutation(k)
    arrays = []
    for i in order:
        n = lens[i]
        s = int(rng.integers(0, len(iq) - n + 1))
        arrays.append(to_format(fmt, iq[s:s + n]))
    return arrays


@pytest.mark.parametrize("fs", [2e6, 8e6, 12e6])
@pytest.mark.parametrize("fmt", [N.FMT_FC32, N.FMT_MAG2, N.FMT_SC16, N.FMT_SC8, N.FMT_CU8])
def test_random_batches_equal_a_loop_of_single_calls(native, fmt, fs):
    rng = np.random.default_rng(1000 * fmt + int(fs // 1e6))
    ctx, ref = make_ctx(fs), make_ctx(fs)
    total = 0
    for k in (1, 2, 63, 257, 1500):
        arrays = random_items(fs, fmt, k, rng)
        thrs = np.where(rng.random(k) < 0.8, 0.01, rng.choice([0.02, 0.005, 0.05], size=k)).astype(np.float32)
        offs = rng.integers(0, 1 << 40, size=k)
        for scattered in (False, True):
            items = DeviceItems(ctx, fmt, arrays, scattered=scattered, seed=k)
            recs, first = ctx.process_batch_device(fmt, items.ptrs, items.ns, thrs, offs)
            assert ctx.last_batch_fallbacks == 0
            want, wfirst = loop(ref, fmt, items, thrs, offs)
            assert np.array_equal(first, wfirst), (k, scattered)
            assert recs.tobytes() == want.tobytes(), (k, scattered)
            total += len(recs)
            items.free()
    assert total > 1000
    ctx.close()
    ref.close()


# ---- 3. power-of-two scales: the loop runs the dot-product instances of k_detect, the batch the generic conversion -----------
@pytest.mark.parametrize("fmt,scale", [(N.FMT_SC8, 2.0 ** -7), (N.FMT_CU8, 2.0 ** -6)])
def test_power_of_two_scale_8bit(native, fmt, scale):
    rng = np.random.default_rng(5)
    sc = {fmt: scale}
    thr = 0.01 if fmt == N.FMT_SC8 else 0.04
    ctx, ref = make_ctx(2e6, thr, scales=sc), make_ctx(2e6, thr, scales=sc)
    # (rise storms short enough for the batch path's first list capacity: a matched centre every ~50 samples against
    # chunk/256 + 64 slots per list)
    arrays = [helpers.rise_storm_iq8(n, seed=i, offset_binary=(fmt == N.FMT_CU8)) for i, n in enumerate((8192, 4096, 2048, 1024))]
    arrays += random_items(2e6, fmt, 150, rng, max_log2=17)
    items = DeviceItems(ctx, fmt, arrays)
    thrs = [thr] * len(arrays)
    recs, first = ctx.process_batch_device(fmt, items.ptrs, items.ns, thrs)
    assert ctx.last_batch_fallbacks == 0
    want, wfirst = loop(ref, fmt, items, thrs)
    assert len(want) > 300 and np.array_equal(first, wfirst) and recs.tobytes() == want.tobytes()
    items.free()
    ctx.close()
    ref.close()


# ---- 4. fallbacks -------------------------------------------------------------------------------------------------------
def test_fallback_items_take_the_ordinary_pass(native):
    fs, fmt = 2e6, N.FMT_FC32
    rng = np.random.default_rng(9)
    ctx, ref = make_ctx(fs), make_ctx(fs)
    ordinary = random_items(fs, fmt, 12, rng, max_log2=16)
    # a centre every 64 samples (helpers.preamble_train_iq) against the batch path's chunk/256 + 64 slots per list and four
    # lists per item: 2^17 samples are 2048 centres for 4 * (32768/256 + 64) = 768 slots
    train = helpers.preamble_train_iq(1 << 17)
    iq = pool(fs)
    long_item = np.tile(iq, 3)[:N.BATCH_ITEM_MAX + 4096]
    arrays = ordinary[:5] + [long_item] + ordinary[5:8] + [train] + ordinary[8:]
    thrs = [0.01] * len(arrays)
    items = DeviceItems(ctx, fmt, arrays)
    recs, first = ctx.process_batch_device(fmt, items.ptrs, items.ns, thrs)
    assert ctx.last_batch_fallbacks == 2
    want, wfirst = loop(ref, fmt, items, thrs)
    assert np.array_equal(first, wfirst) and recs.tobytes() == want.tobytes()
    assert first[6] - first[5] > 1000 and first[10] - first[9] > 100      # the two fallback items delivered their records
    items.free()
    # without them: none
    items = DeviceItems(ctx, fmt, ordinary)
    recs, first = ctx.process_batch_device(fmt, items.ptrs, items.ns, thrs[:len(ordinary)])
    assert ctx.last_batch_fallbacks == 0
    want, wfirst = loop(ref, fmt, items, thrs)
    assert np.array_equal(first, wfirst) and recs.tobytes() == want.tobytes()
    items.free()
    ctx.close()
    ref.close()


def test_fallback_items_leave_the_last_result_alone(native):
    """adsb_last_result after a batch is what it was before it, fallback items or not: the fallback passes run in a pipeline
    slot other than the one the last result lives in, and the context's threshold is put back."""
    fs, fmt = 2e6, N.FMT_FC32
    rng = np.random.default_rng(21)
    ctx, ref = make_ctx(fs), make_ctx(fs)
    iq = pool(fs)
    train = helpers.preamble_train_iq(1 << 17)                       # overflows the batch path's lists (see above)
    long_item = np.tile(iq, 3)[:N.BATCH_ITEM_MAX + 4096]
    ordinary = random_items(fs, fmt, 6, rng, max_log2=16)
    arrays = ordinary[:3] + [train] + ordinary[3:] + [long_item]
    items = DeviceItems(ctx, fmt, arrays + [iq[:200000]])
    bp, bn = items.ptrs[:-1], items.ns[:-1]
    thrs = [0.02] * len(arrays)
    want_last = ref.process_format_device(fmt, items.ptrs[-1], items.ns[-1], 5)
    assert len(want_last) > 100
    # (a) after a blocking call; (b) after a submitted pass in every pipeline slot
    for before in ("blocking", "ticket0", "ticket1", "ticket2"):
        if before == "blocking":
            n_before = ctx.process_format_device(fmt, items.ptrs[-1], items.ns[-1], 5, fetch=False)
        else:
            for _ in range(int(before[-1])):                        # move on to the next slot
                ctx.wait(ctx.submit_format_device(fmt, items.ptrs[0], items.ns[0]), fetch=False)
            n_before = ctx.wait(ctx.submit_format_device(fmt, items.ptrs[-1], items.ns[-1], 5), fetch=False)
        assert n_before == len(want_last)
        view = ctx.last_result(copy=False)                          # a zero-copy view into the slot's pinned buffer
        recs, first = ctx.process_batch_device(fmt, bp, bn, thrs)
        assert ctx.last_batch_fallbacks == 2
        assert first[4] - first[3] > 100 and first[-1] - first[-2] > 1000
        assert view.tobytes() == want_last.tobytes(), before
        assert ctx.last_result().tobytes() == want_last.tobytes(), before
        # ... and the context's own threshold (0.01) is what the next call runs with
        assert ctx.process_format_device(fmt, items.ptrs[-1], items.ns[-1], 5).tobytes() == want_last.tobytes()
    ref.set_threshold(0.02)
    want = np.concatenate([ref.process_format_device(fmt, p, n) for p, n in zip(bp, bn)])
    assert recs.tobytes() == want.tobytes()
    items.free()
    ctx.close()
    ref.close()


# ---- 5. host variant -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [N.FMT_FC32, N.FMT_CU8])
def test_host_variant_equals_the_device_variant(native, fmt):
    fs = 2e6
    rng = np.random.default_rng(77)
    ctx = make_ctx(fs)
    arrays = random_items(fs, fmt, 70, rng, max_log2=17)
    if fmt == N.FMT_CU8:
        arrays.append(to_format(fmt, np.tile(pool(fs), 5)[:(9 << 20) + 6]))        # larger than a staging chunk (16 MiB)
    thrs = rng.choice([0.01, 0.02], size=len(arrays)).astype(np.float32)
    offs = rng.integers(0, 1 << 30, size=len(arrays))
    items = DeviceItems(ctx, fmt, arrays)
    want, wfirst = ctx.process_batch_device(fmt, items.ptrs, items.ns, thrs, offs)
    assert ctx.last_batch_fallbacks == expected_fallbacks(items.ns) and len(want) > 100
    items.free()
    got, first = ctx.process_batch(fmt, arrays, thrs, offs)                           # pageable
    assert ctx.last_batch_fallbacks == expected_fallbacks(items.ns)
    assert np.array_equal(first, wfirst) and got.tobytes() == want.tobytes()
    pinned = []
    for k, a in enumerate(arrays):                                                    # page-locked, and mixed with pageable
        if k % 3 == 2:
            pinned.append(a)
            continue
        p = N.PinnedArray(max(len(a), 1), a.dtype, near=ctx)
        p.array[:len(a)] = a
        pinned.append(p)
    got, first = ctx.process_batch(fmt, [p if isinstance(p, np.ndarray) else p.array[:len(arrays[k])] for k, p in enumerate(pinned)],
                                   thrs, offs)
    assert ctx.last_batch_fallbacks == expected_fallbacks(items.ns)
    assert np.array_equal(first, wfirst) and got.tobytes() == want.tobytes()
    ctx.close()


# ---- 6. context flags that apply to every item --------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [N.FLAG_FEC_CONSERVATIVE, N.FLAG_LONG_AWARE_GATE, N.FLAG_FEC_CONSERVATIVE | N.FLAG_LONG_AWARE_GATE])
def test_fec_and_long_aware_contexts(native, flags):
    from test_gpu_fec import stream, THR
    from test_fec import GOLDEN
    golden = np.load(GOLDEN)
    fs = 2e6
    iq, starts = stream(golden, fs)
    ctx, ref = make_ctx(fs, THR, flags=flags), make_ctx(fs, THR, flags=flags)
    # the rows' stream cut between replies into items of unequal length, plus the whole stream as one item
    cuts = [0] + [int(starts[k]) - 100 for k in (7, 8, 40, 100, len(starts) // 2)] + [len(iq)]
    arrays = [iq[a - a % 2:b - b % 2] for a, b in zip(cuts[:-1], cuts[1:])] + [iq]
    for fmt in (N.FMT_FC32, N.FMT_SC16):
        data = [to_format(fmt, a) for a in arrays]
        items = DeviceItems(ctx, fmt, data)
        thrs = [THR] * len(data)
        recs, first = ctx.process_batch_device(fmt, items.ptrs, items.ns, thrs)
        assert ctx.last_batch_fallbacks == 0
        want, wfirst = loop(ref, fmt, items, thrs)
        assert np.array_equal(first, wfirst) and recs.tobytes() == want.tobytes()
        if flags & N.FLAG_FEC_CONSERVATIVE:
            assert np.count_nonzero(recs["flags"] & N.BURST_FEC_FIXED) > 0
        else:
            assert not np.any(recs["flags"] & N.BURST_FEC_FIXED)
        items.free()
    ctx.close()
    ref.close()


# ---- 7. refusals and edges ---------------------------------------------------------------------------------------------------
def _raw_call(ctx, fmt, items, out, first, cap=None, fn=None):
    n_out, n_fb = ctypes.c_int32(-5), ctypes.c_int32(-5)
    fn = fn or ctx.lib.adsb_process_batch_device
    rc = fn(ctx._h, int(fmt), ctypes.c_void_p(items.ctypes.data), len(items), ctypes.c_void_p(out.ctypes.data),
            len(out) if cap is None else cap, ctypes.c_void_p(first.ctypes.data), ctypes.byref(n_out), ctypes.byref(n_fb))
    return rc, n_out.value, n_fb.value


def _item_table(di, thr=0.01):
    t = np.zeros(len(di.ptrs), dtype=N.BATCH_ITEM_DTYPE)
    t["data"], t["n"], t["threshold"] = di.ptrs, di.ns, thr
    return t


def test_refusals_and_edges(native):
    fs, fmt = 2e6, N.FMT_FC32
    rng = np.random.default_rng(3)
    ctx = make_ctx(fs)
    arrays = random_items(fs, fmt, 40, rng, max_log2=17)
    di = DeviceItems(ctx, fmt, arrays)
    table = _item_table(di)
    out = np.zeros(1 << 14, dtype=N.BURST_DTYPE)
    first = np.zeros(len(table) + 1, dtype=np.int32)
    rc, n, fb = _raw_call(ctx, fmt, table, out, first)
    assert rc == 0 and n > 20 and fb == 0 and first[-1] == n
    good = out[:n].copy()
    # cap one short: -ENOSPC and the number needed; a second call with that capacity succeeds
    out2 = np.zeros(n, dtype=N.BURST_DTYPE)
    rc, n2, _ = _raw_call(ctx, fmt, table, out2, first, cap=n - 1)
    assert rc == -ENOSPC and n2 == n
    rc, n2, _ = _raw_call(ctx, fmt, table, out2, first)
    assert rc == 0 and n2 == n and out2.tobytes() == good.tobytes()
    # no items
    rc, n0, fb = _raw_call(ctx, fmt, table[:0], out, first)
    assert rc == 0 and n0 == 0 and fb == 0 and first[0] == 0
    r, f = ctx.process_batch_device(fmt, [], [])
    assert len(r) == 0 and list(f) == [0]
    # reserved != 0, n < 0, a misaligned pointer, a bad format
    for field, val in (("reserved", 1), ("n", -1)):
        bad = table.copy()
        bad[field][4] = val
        assert _raw_call(ctx, fmt, bad, out, first)[0] == -EINVAL
    bad = table.copy()
    bad["data"][2] += 8
    assert _raw_call(ctx, fmt, bad, out, first)[0] == -EINVAL
    assert _raw_call(ctx, 5, table, out, first)[0] == -EINVAL
    assert _raw_call(ctx, -1, table, out, first)[0] == -EINVAL
    # the host variant checks the same
    assert _raw_call(ctx, fmt, bad, out, first, fn=ctx.lib.adsb_process_batch)[0] == -EINVAL
    # a pending ticket
    t = ctx.submit_format_device(fmt, di.ptrs[0], di.ns[0])
    assert _raw_call(ctx, fmt, table, out, first)[0] == -EBUSY
    ctx.wait(t)
    rc, n2, _ = _raw_call(ctx, fmt, table, out2, first)
    assert rc == 0 and out2.tobytes() == good.tobytes()
    # contexts that model ONE receiver
    for fl in (N.FLAG_AIRCRAFT_TABLE, N.FLAG_DECODE | N.FLAG_AIRCRAFT_TABLE, N.FLAG_CONFIDENCE):
        c2 = make_ctx(fs, flags=fl)
        assert _raw_call(c2, fmt, table, out, first)[0] == -EINVAL
        assert _raw_call(c2, fmt, table, out, first, fn=c2.lib.adsb_process_batch)[0] == -EINVAL
        c2.close()
    # a timed context is accepted; the batch kernel does not feed the detect_* statistics
    c3 = make_ctx(fs, flags=N.FLAG_TIMING)
    rc, n3, fb = _raw_call(c3, fmt, table, out2, first)
    assert rc == 0 and fb == 0 and out2[:n3].tobytes() == good.tobytes() and c3.stats()["detect_launches"] == 0
    c3.close()
    di.free()
    ctx.close()


# ---- 8. the context afterwards -------------------------------------------------------------------------------------------------
def test_a_batch_call_leaves_the_context_as_it_was(native):
    fs = 2e6
    rng = np.random.default_rng(12)
    x = M.mag2(pool(fs))
    arrays = random_items(fs, N.FMT_MAG2, 20, rng, max_log2=16)

    def session(with_batch):
        ctx = make_ctx(fs)
        di = DeviceItems(ctx, N.FMT_MAG2, arrays + [x[:300000]])
        got = []

        def batch():
            if with_batch:
                r, f = ctx.process_batch_device(N.FMT_MAG2, di.ptrs[:-1], di.ns[:-1], [0.02] * len(arrays))
                assert ctx.last_batch_fallbacks == 0 and len(r) > 0

        tk = [ctx.submit_format_device(N.FMT_MAG2, di.ptrs[-1] + 4 * 4000 * i, 100000, i) for i in range(3)]
        got += [ctx.wait(t) for t in tk]
        batch()
        tk = [ctx.submit_format_device(N.FMT_MAG2, di.ptrs[-1] + 4 * 4000 * i, 120000, i) for i in range(3)]
        got += [ctx.wait(t) for t in tk]
        # GNU Radio emulation: framer.work() calls with history, state carried from call to call
        H = 8 * 2 - 1
        pos, hist = 0, np.zeros(H, dtype=np.float32)
        for k, N_ in enumerate((4096, 3000, 8192, 1000, 4096)):
            in0 = np.concatenate([hist, x[pos:pos + N_]])
            got.append(ctx.framer_work(in0, N_, pos))
            got.append(np.array(ctx.framer_state(), dtype=np.float64))
            hist = in0[-H:]
            pos += N_
            if k in (1, 3):
                batch()
                assert np.array(ctx.framer_state(), dtype=np.float64).tobytes() == got[-1].tobytes()
        di.free()
        ctx.close()
        return got

    a, b = session(False), session(True)
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert sum(len(u) for u in a if u.dtype == N.BURST_DTYPE) > 100


# ---- 9. the RTL-SDR fleet ------------------------------------------------------------------------------------------------------
def test_1024_receivers_of_uint8_iq_against_the_c_oracle(native):
    from oracle import adsb_oracle as O
    from oracle import c_oracle
    fs, fmt, n = 2e6, N.FMT_CU8, 1 << 16
    scale = float(np.float32(FMT_SCALE[fmt]))
    u8 = to_format(fmt, np.tile(pool(fs), 3)).reshape(-1, 2)
    rng = np.random.default_rng(1024)
    starts = rng.integers(0, len(u8) - n, size=1024) // 8 * 8
    ctx = make_ctx(fs)
    # one allocation holding the pool; the items are 1024 (overlapping) windows of it
    base = ctx.device_alloc(u8.nbytes)
    ctx.device_upload(base, u8)
    ptrs = [base + 2 * int(s) for s in starts]
    recs, first = ctx.process_batch_device(fmt, ptrs, [n] * 1024)
    assert ctx.last_batch_fallbacks == 0 and len(first) == 1025
    total = 0
    for i, s in enumerate(starts):
        x = O.mag2_iq8(u8[s:s + n].reshape(-1), scale, True)
        want = c_oracle.canonical(x, 2, 0.01)
        helpers.assert_recs_equal(recs[first[i]:first[i + 1]], want, "receiver %d" % i)
        total += len(want)
    assert total > 50000
    ctx.device_free(base)
    ctx.close()
