"""adsb_process_stream_batch* on the MI355X: receiver streams carried across batch calls (k_stream_stage, k_batch, k_batch_pack,
k_stream_save) against the reference's single-call vectors, against adsb_process_format over each stream's whole input on a
second context, and against the C oracle.  Every comparison is byte for byte, and wherever equality is claimed the streams'
overlong counts are asserted 0.  The CPU half (emulator) is tests/test_stream_batch.py."""
import numpy as np
import pytest

import helpers
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend
from gr_adsb_amd import modulator as M

pytestmark = pytest.mark.gpu

ENOSPC, EBUSY, EINVAL = 28, 16, 22
EMPTY = np.zeros(0, dtype=N.BURST_DTYPE)


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N.load()
    return N


def cuts_fixed(n, step):
    return [min(step, n - a) for a in range(0, n, step)]


def cuts_random(n, hi, seed, specials=(0, 1, 3, 0, 255)):
    """chunk lengths 0..hi that sum to n, with zero, one, odd and short lengths mixed in first"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    for s in specials:
        for v in (int(rng.integers(0, hi + 1)), s):
            v = min(v, left)
            out.append(v)
            left -= v
    while left > 0:
        v = min(int(rng.integers(0, hi + 1)), left)
        out.append(v)
        left -= v
    return out


def cat(parts):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else EMPTY.copy()


def drive(ctx, fmt, sources, cuts, thrs, device=False, ids=None):
    """sources[i]: stream i's whole input in the format's layout; cuts[i]: its chunk lengths.  One call per round pushes the
    next chunk of every stream that still has one (streams run out at different times), a last call ends them all.
    device: the sources lie in device memory and the chunks are read where they lie (any sample alignment).
    -> per stream: the concatenated records; the number of fallback items seen"""
    per = N.FMT_LAYOUT[fmt][1]
    bps = N.FMT_BYTES[fmt]
    k = len(sources)
    ids = list(range(k)) if ids is None else ids
    pos, nxt, got, nfb = [0] * k, [0] * k, [[] for _ in range(k)], 0
    bases = []
    if device:
        for s in sources:
            b = ctx.device_alloc(max(s.nbytes, 16))
            ctx.device_upload(b, np.ascontiguousarray(s))
            bases.append(b)
    while any(nxt[i] < len(cuts[i]) for i in range(k)):
        live = [i for i in range(k) if nxt[i] < len(cuts[i])]
        ns = [cuts[i][nxt[i]] for i in live]
        th = [thrs[i] for i in live]
        if device:
            recs, first = ctx.process_stream_batch_device(fmt, [ids[i] for i in live], [bases[i] + pos[i] * bps for i in live], ns, th)
        else:
            recs, first = ctx.process_stream_batch(fmt, [ids[i] for i in live],
                                                   [sources[i][pos[i] * per:(pos[i] + n) * per] for i, n in zip(live, ns)], th)
        nfb += ctx.last_batch_fallbacks
        for j, i in enumerate(live):
            got[i].append(recs[first[j]:first[j + 1]])
            pos[i] += ns[j]
            nxt[i] += 1
            assert ctx.stream_state(ids[i])[0] == pos[i]
    dt = N.FMT_LAYOUT[fmt][0]
    recs, first = ctx.process_stream_batch(fmt, ids, [np.zeros(0, dtype=dt)] * k, thrs, end=True)
    nfb += ctx.last_batch_fallbacks
    for i in range(k):
        assert pos[i] * per == len(sources[i])
        got[i].append(recs[first[i]:first[i + 1]])
        assert ctx.stream_state(ids[i])[:2] == (0, N.STREAM_FRESH_EOB)
    for b in bases:
        ctx.device_free(b)
    return [cat(g) for g in got], nfb


# ---- 1. the reference's single-call vectors, both entry points ---------------------------------------------------------
_GOLD = {2: ("g2msps_df17", "L2msps_df17"), 8: ("g8msps_dense", "L8msps_dense"), 20: ("g20msps", "L20msps")}


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("sps", [2, 8, 20])
def test_goldens_as_streams(native, sps, device):
    g = helpers.Golden(_GOLD[sps][0])
    big = helpers.Golden(_GOLD[sps][1])
    n = len(g.x)
    F = 256 + 121 * sps
    cuts = [cuts_fixed(n, 4096), g.sched("random"), cuts_random(n, 3000, seed=11), cuts_random(n, 70000, seed=12),
            [F - 1, 1, F, 5] + cuts_fixed(n - 2 * F - 5, 8192)]
    ctx = N.Context(g.fs, g.thr)
    ctx.set_format_scale(N.FMT_SC16, 2.0 / 32767.0)
    ctx.set_format_scale(N.FMT_SC8, float(big.scale))
    ctx.open_streams(8)
    for fmt, src in ((N.FMT_MAG2, np.asarray(g.x, dtype=np.float32)), (N.FMT_FC32, g.iq), (N.FMT_SC16, g.z["iq16"])):
        got, nfb = drive(ctx, fmt, [src] * len(cuts), cuts, [g.thr] * len(cuts), device=device, ids=[7, 0, 3, 2, 5])
        assert nfb == 0
        for r in got:
            helpers.assert_recs_match_golden(r, g, "single")
    nb = len(big.x)
    bcuts = [cuts_random(nb, 70000, seed=5), cuts_fixed(nb, 65536 + 3), cuts_fixed(nb, (1 << 18) + 1)]
    got, nfb = drive(ctx, N.FMT_SC8, [big.iq8] * 3, bcuts, [big.thr] * 3, device=device)
    assert nfb == 0
    for r in got:
        helpers.assert_recs_match_golden(r, big, "single")
    assert all(ctx.stream_state(i)[2] == 0 for i in range(8))          # the condition under which equality is claimed
    ctx.close()


@pytest.mark.parametrize("device", [False, True])
def test_uint8_byte_pairs_against_the_c_oracle(native, device):
    """Offset-binary uint8 (no byte converts to 0: a fresh stream's buffer must start AT the stream, with nothing in front):
    three windows of every_byte_pair_stream -- bursts from the first samples on -- as streams, against the C oracle on the
    oracle's own conversion."""
    from oracle import adsb_oracle as O
    from oracle import c_oracle as C
    scale = float(np.float32(3.0 / 256.0))
    iq8, _ = helpers.every_byte_pair_stream(1.0, quiet=0x8080)
    u8 = iq8.view(np.uint8)
    thr = np.float32(6.0) * np.float32(scale) * np.float32(scale)
    n = 1 << 19
    starts = [0, 20 + 5000 * 256, len(u8) // 2 - n]                 # window 1 starts inside a slot's noise window: high at once
    srcs = [np.ascontiguousarray(u8[2 * s:2 * (s + n)]) for s in starts]
    cuts = [cuts_random(n, 70000, seed=31), cuts_fixed(n, 4097), cuts_random(n, 3000, seed=32)]
    ctx = N.Context(2e6, float(thr))
    ctx.set_format_scale(N.FMT_CU8, scale)
    ctx.open_streams(3)
    got, nfb = drive(ctx, N.FMT_CU8, srcs, cuts, [float(thr)] * 3, device=device)
    assert nfb == 0
    for i, r in enumerate(got):
        want = C.canonical(O.mag2_iq8(srcs[i], scale, True), 2, thr)
        assert len(want) > 1500
        helpers.assert_recs_equal(r, want, "window %d" % i)
        assert ctx.stream_state(i)[2] == 0
    ctx.close()


# ---- 2. a fleet ----------------------------------------------------------------------------------------------------------
def _fleet(sps, count, seed):
    g = helpers.Golden({2: "L2msps_df17", 8: "L8msps_dense"}[sps])
    rng = np.random.default_rng(seed)
    pairs = g.iq8.reshape(-1, 2)
    srcs = []
    for _ in range(count):
        n = int(rng.integers(20000, 200000))
        s = int(rng.integers(0, len(pairs) - n))
        srcs.append(np.ascontiguousarray(pairs[s:s + n]).reshape(-1))
    return g, srcs


@pytest.mark.parametrize("sps", [2, 8])
def test_a_fleet_of_200_streams_under_two_chunkings(native, sps):
    g, srcs = _fleet(sps, 200, seed=200 + sps)
    ref = N.Context(g.fs, g.thr)
    ref.set_format_scale(N.FMT_SC8, float(g.scale))
    want = [ref.process_format(N.FMT_SC8, s) for s in srcs]
    ref.close()
    assert sum(len(w) for w in want) > 5000
    fe = frontend.FrontEnd(g.fs, g.thr)
    fe.ctx.set_format_scale(N.FMT_SC8, float(g.scale))
    rx = fe.receivers(200)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        pos = [0] * 200
        got = [[] for _ in range(200)]
        while True:
            live = [i for i in range(200) if pos[i] * 2 < len(srcs[i])]
            if not live:
                break
            ns = [int(rng.integers(0, 70001)) for _ in live]
            parts = rx.push([srcs[i][2 * pos[i]:2 * (pos[i] + n)] for i, n in zip(live, ns)], ids=live)
            assert fe.last_batch_fallbacks == 0
            for i, n, r in zip(live, ns, parts):
                got[i].append(r)
                pos[i] = min(pos[i] + n, len(srcs[i]) // 2)
        for i, r in enumerate(rx.finish()):
            got[i].append(r)
            helpers.assert_recs_equal(cat(got[i]), want[i], "stream %d, chunking %d" % (i, seed))
        assert rx.overlong == 0
    rx.close()
    fe.ctx.close()


# ---- 3. fallback, retry ----------------------------------------------------------------------------------------------------
def test_a_chunk_over_the_item_limit_takes_the_ordinary_pass(native):
    fs = 2e6
    iq = M.synth_iq(N.BATCH_ITEM_MAX + (1 << 17) + 12345, fs, 4000, 77)
    x = M.mag2(iq)
    a, b = 50001, 50001 + N.BATCH_ITEM_MAX + 4096
    ctx = N.Context(fs, 0.01)
    want = ctx.process_format(N.FMT_MAG2, x)
    ctx.open_streams(2)
    small = x[:30000]
    got, fbs = [], []
    for lo, hi in ((0, a), (a, b), (b, len(x))):
        recs, first = ctx.process_stream_batch(N.FMT_MAG2, [1, 0], [small if lo == 0 else small[:0], x[lo:hi]])
        fbs.append(ctx.last_batch_fallbacks)
        got.append(recs[first[1]:first[2]])
    recs, first = ctx.process_stream_batch(N.FMT_MAG2, [0], [x[:0]], end=True)
    got.append(recs)
    assert fbs == [0, 1, 0]
    helpers.assert_recs_equal(cat(got), want, "a chunk longer than ADSB_BATCH_ITEM_MAX in the middle of a stream")
    assert cat(got).tobytes() == want.tobytes() and ctx.stream_state(0)[2] == 0 and len(want) > 3000
    ctx.close()


def test_enospc_moves_nothing_and_the_call_can_be_repeated(native):
    g = helpers.Golden("g2msps_df17")
    x = np.asarray(g.x, dtype=np.float32)
    ctx = N.Context(g.fs, g.thr)
    ctx.open_streams(2)
    r0, _ = ctx.process_stream_batch(N.FMT_MAG2, [0, 1], [x[:40000], x[:999]])
    before = [ctx.stream_state(i) for i in (0, 1)]
    with pytest.raises(N.AdsbError) as e:
        ctx.process_stream_batch(N.FMT_MAG2, [0, 1], [x[40000:90000], x[999:70000]], cap=3)
    assert e.value.code == -ENOSPC and ctx.last_stream_needed > 3
    assert [ctx.stream_state(i) for i in (0, 1)] == before
    r1, f1 = ctx.process_stream_batch(N.FMT_MAG2, [0, 1], [x[40000:90000], x[999:70000]], cap=ctx.last_stream_needed)
    assert len(r1) == ctx.last_stream_needed
    r2, f2 = ctx.process_stream_batch(N.FMT_MAG2, [0, 1], [x[90000:], x[70000:]], end=True)
    # the same pushes on a context that always had room
    c2 = N.Context(g.fs, g.thr)
    c2.open_streams(2)
    s0, _ = c2.process_stream_batch(N.FMT_MAG2, [0, 1], [x[:40000], x[:999]])
    s1, g1 = c2.process_stream_batch(N.FMT_MAG2, [0, 1], [x[40000:90000], x[999:70000]])
    s2, g2 = c2.process_stream_batch(N.FMT_MAG2, [0, 1], [x[90000:], x[70000:]], end=True)
    assert (r0.tobytes(), r1.tobytes(), r2.tobytes()) == (s0.tobytes(), s1.tobytes(), s2.tobytes())
    assert list(f1) == list(g1) and list(f2) == list(g2)
    f0 = [0, len(r0), len(r0)]                      # (stream 1's first 999 samples are still inside its look-ahead)
    for i in (0, 1):
        helpers.assert_recs_match_golden(cat([r0[f0[i]:f0[i + 1]], r1[f1[i]:f1[i + 1]], r2[f2[i]:f2[i + 1]]]), g, "single")
    ctx.close()
    c2.close()


# ---- 4. refusals, resets, other state -------------------------------------------------------------------------------------
def _code(fn, *a, **k):
    with pytest.raises(N.AdsbError) as e:
        fn(*a, **k)
    return e.value.code


def test_refusals(native):
    x = M.mag2(M.synth_iq(20000, 2e6, 4000, 3))
    ctx = N.Context(2e6, 0.01)
    assert _code(ctx.process_stream_batch, N.FMT_MAG2, [0], [x]) == -EINVAL            # no streams open
    ctx.open_streams(3)
    assert _code(ctx.open_streams, 3) == -EINVAL
    assert _code(ctx.process_stream_batch, N.FMT_MAG2, [1, 1], [x, x]) == -EINVAL      # a stream twice
    assert _code(ctx.process_stream_batch, N.FMT_MAG2, [3], [x]) == -EINVAL            # out of range
    assert _code(ctx.process_stream_batch, N.FMT_MAG2, [-1], [x]) == -EINVAL
    ctx.process_stream_batch(N.FMT_MAG2, [0], [x])
    assert _code(ctx.process_stream_batch, N.FMT_FC32, [0], [x[:100].astype(np.complex64)]) == -EINVAL      # another format mid-stream
    assert _code(ctx.set_stream_base, 0, 5) == -EINVAL                                 # not fresh
    d = ctx.device_alloc(1 << 16)
    assert _code(ctx.process_stream_batch_device, N.FMT_MAG2, [1], [d + 2], [100]) == -EINVAL         # not aligned to a sample
    items = np.zeros(1, dtype=N.STREAM_ITEM_DTYPE)
    items["data"], items["n"], items["stream"], items["threshold"] = d, 100, 1, 0.01
    out = np.zeros(64, dtype=N.BURST_DTYPE)
    first = np.zeros(2, dtype=np.int32)
    import ctypes
    n_out, n_fb = ctypes.c_int32(0), ctypes.c_int32(0)

    def raw():
        return ctx.lib.adsb_process_stream_batch_device(ctx._h, N.FMT_MAG2, ctypes.c_void_p(items.ctypes.data), 1,
                                                        ctypes.c_void_p(out.ctypes.data), 64, ctypes.c_void_p(first.ctypes.data),
                                                        ctypes.byref(n_out), ctypes.byref(n_fb))
    items["reserved"] = 1
    assert raw() == -EINVAL
    items["reserved"], items["flags"] = 0, 2
    assert raw() == -EINVAL
    items["flags"], items["n"] = 0, -1
    assert raw() == -EINVAL
    # pending tickets
    t = ctx.submit_format_device(N.FMT_MAG2, d, 1 << 14)
    assert _code(ctx.process_stream_batch, N.FMT_MAG2, [1], [x]) == -EBUSY
    ctx.wait(t)
    assert ctx.stream_state(0)[0] == len(x) and ctx.stream_state(1)[0] == 0           # nothing moved by the refused calls
    ctx.device_free(d)
    ctx.close()
    for fl in (N.FLAG_AIRCRAFT_TABLE, N.FLAG_AIRCRAFT_TABLE | N.FLAG_DECODE, N.FLAG_CONFIDENCE):
        c = N.Context(2e6, 0.01, flags=fl)
        assert _code(c.open_streams, 2) == -EINVAL
        assert _code(c.process_stream_batch, N.FMT_MAG2, [0], [x]) == -EINVAL
        c.close()


def test_resets_make_streams_fresh(native):
    g = helpers.Golden("g2msps_df17")
    x = np.asarray(g.x, dtype=np.float32)
    ctx = N.Context(g.fs, g.thr)
    ctx.open_streams(2)
    ctx.set_stream_base(1, 1000)
    for how in ("stream", "context"):
        ctx.process_stream_batch(N.FMT_MAG2, [0, 1], [x[:50000], x[:7777]])
        assert ctx.stream_state(0)[0] == 50000 and ctx.stream_state(0)[1] != N.STREAM_FRESH_EOB
        if how == "stream":
            ctx.reset_stream(0)
            assert ctx.stream_state(1)[0] == 7777
            ctx.reset_stream(1)
        else:
            ctx.reset()
        assert [ctx.stream_state(i)[:2] for i in (0, 1)] == [(0, N.STREAM_FRESH_EOB)] * 2
        recs, first = ctx.process_stream_batch(N.FMT_MAG2, [0, 1], [x, x], end=True)          # another format would be fine too
        helpers.assert_recs_match_golden(recs[:first[1]], g, "single")
        r1 = recs[first[1]:].copy()
        r1["offset"] -= 1000                                                                  # the base stays
        helpers.assert_recs_match_golden(r1, g, "single")
    ctx.close()


def test_fec_and_long_aware_contexts_and_untouched_state(native):
    g = helpers.Golden("g2msps_mixed_lowsnr")
    x = np.asarray(g.x, dtype=np.float32)
    n = len(x)
    for fl in (N.FLAG_FEC_CONSERVATIVE, N.FLAG_LONG_AWARE_GATE, N.FLAG_FEC_CONSERVATIVE | N.FLAG_LONG_AWARE_GATE):
        ctx = N.Context(g.fs, g.thr, flags=fl)
        want = ctx.process_format(N.FMT_MAG2, x)
        if fl & N.FLAG_FEC_CONSERVATIVE:
            assert np.any(want["flags"] & N.BURST_FEC_FIXED)
        # a framer call and a canonical call leave state that the stream batch must not touch
        ctx.framer_work(x[:5000], 5000 - (8 * g.sps - 1), 0)
        keep = ctx.process_format(N.FMT_MAG2, x[:30000])
        st = ctx.framer_state()
        ctx.open_streams(2)
        got, nfb = drive(ctx, N.FMT_MAG2, [x, x], [cuts_random(n, 9000, seed=8), cuts_fixed(n, 5000)], [g.thr] * 2)
        assert nfb == 0
        for r in got:
            assert r.tobytes() == want.tobytes()
        assert ctx.framer_state() == st and ctx.last_result().tobytes() == keep.tobytes()
        ctx.close()


# ---- 5. lifecycle ----------------------------------------------------------------------------------------------------------
def test_lifecycle_releases_the_stream_buffers(native):
    import torch
    fs = 2e6
    iq = M.synth_iq(1 << 20, fs, 4000, 61)
    items = [iq[k << 17:(k + 1) << 17].copy() for k in range(8)]

    def use():
        ctx = N.Context(fs, 0.01)
        ctx.open_streams(64)
        got, _ = ctx.process_stream_batch(N.FMT_FC32, list(range(8)), items)
        more, _ = ctx.process_stream_batch(N.FMT_FC32, list(range(8)), items, end=True)
        assert len(got) + len(more) > 1000
        ctx.close_streams()
        ctx.open_streams(8)
        ctx.process_stream_batch(N.FMT_FC32, [0], [items[0]])
        ctx.close()                                   # with streams open: adsb_destroy releases them

    free = []
    for rep in range(31):
        use()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[10] - free[30] < (16 << 20), [(f - free[0]) >> 20 for f in free]
