"""The burst-record routes of tests/burst_paths.py on the GPU, through the C ABI: long-pulse bursts (k_longrun:
burst_issue / burst_finish, fast and clipped), full pending lists and pend_flush in k_detect, for all five formats (int8
at its default scale runs the dot-product instance k_detect<5, .>, uint8 also at 2^-7: k_detect<6, .>), host,
device-resident, submitted and sharded entry points, bit for bit against the C oracle on the oracle's |IQ|^2 of the same
bytes; the fused path's confidence ratios; the drop-in framer with the paired and with the stand-alone demod against the
reference fixtures tests/golden/Qpaths_*.npz; and adsb_demod_work (k_slice) at its edges, with and without
ADSB_FLAG_FEC_CONSERVATIVE."""
import warnings

import numpy as np
import pytest

import burst_paths as B
import edge_cases as E
from helpers import Golden, assert_recs_equal, path_golden_names, schedules_of, unpack
from oracle import adsb_oracle as O
from oracle import c_oracle as C
from test_gpu_parity import native, torch_mod  # noqa: F401  (the module's fixtures)

pytestmark = pytest.mark.gpu

RATES = (2, 4, 8, 20, 6, 12)
INSTANCES = [("fc32", None), ("mag2", None), ("sc16", 1.0 / 32768.0), ("sc8", 1.0 / 128.0), ("sc8", 3.0 / 256.0),
             ("cu8", 1.0 / 255.0), ("cu8", 2.0 ** -7)]


def _dev(torch, data):
    raw = np.ascontiguousarray(data).view(np.uint8)
    return torch.from_numpy(raw.copy()).to("cuda:0")


def _crosses_a_border(native, x, thr, sps, shards):
    """Does a run of the stream cross an owner border of adsb_process_sharded_device's shards (adsb_shard_bounds, align
    4096) by more than the 256 samples of pulse its forward halo follows?  Only then may the call fail with -EOVERFLOW."""
    a = np.r_[False, x >= thr, False]
    d = np.flatnonzero(a[1:] != a[:-1])
    rise, fall = d[0::2], d[1::2]
    for g in range(shards - 1):
        b = native.shard_bounds(len(x), shards, g, sps)[1]
        if np.any((rise < b) & (fall > b + 256)):
            return True
    return False


def _sharded(native, sh, f, ptr, x, thr, sps, want, what):
    """three shards (equal to the canonical call, or -EOVERFLOW if a run crosses a border past the halo), and the largest
    shard count of 8 .. 1 whose borders no such run crosses: that one must succeed.  Returns that count."""
    try:
        assert_recs_equal(sh.process_sharded_device(f, ptr, len(x), 3), want, what + " 3 shards")
    except native.AdsbError as e:
        assert e.code == -75 and _crosses_a_border(native, x, thr, sps, 3), what + " 3 shards: %s" % e
    for shards in range(8, 0, -1):
        if not _crosses_a_border(native, x, thr, sps, shards):
            assert_recs_equal(sh.process_sharded_device(f, ptr, len(x), shards), want, what + " %d shards" % shards)
            return shards
    raise AssertionError("one shard has no border")


@pytest.mark.parametrize("sps", RATES)
@pytest.mark.parametrize("fmt,scale", INSTANCES)
def test_routes_every_entry_point(native, torch_mod, fmt, scale, sps):
    f = E.FORMATS[fmt][0]
    thr = B.threshold(fmt, scale)
    ctx = native.Context(sps * 1e6, thr, flags=native.FLAG_CONFIDENCE)
    sh = native.Context(sps * 1e6, thr)                  # (adsb_process_sharded_device: not for confidence contexts)
    if scale is not None:
        ctx.set_format_scale(f, scale)
        sh.set_format_scale(f, scale)
    n_multi = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, i, q, routes in B.streams(sps):
            data, x = E.encode(fmt, i, q, scale)
            what = "%s %r %d Msps: %s" % (fmt, scale, sps, name)
            want = C.canonical(x, sps, thr)
            before = ctx.stats()["longrun_calls"]
            got = ctx.process_format(f, data)
            assert_recs_equal(got, want, what + " host")
            if routes & {"long_fast", "long_clipped"}:
                assert ctx.stats()["longrun_calls"] > before, what + ": k_longrun did not run"
            # the fused path's confidence ratios: float32 b1 / b0 (demod.py:97-101) of every PDU, as bit patterns
            dem = (got["flags"] & 1) != 0
            _, _, r, _ = O.demod_call(x, sps, 0, got["offset"][dem])
            assert np.array_equal(ctx.last_confidence()[dem].view(np.uint32), r.view(np.uint32)), what + " confidence"
            n = len(x)
            t = _dev(torch_mod, data)
            torch_mod.cuda.synchronize()
            assert_recs_equal(ctx.process_format_device(f, t.data_ptr(), n), want, what + " device")
            assert_recs_equal(ctx.wait(ctx.submit_format_device(f, t.data_ptr(), n)), want, what + " submitted")
            if _sharded(native, sh, f, t.data_ptr(), x, thr, sps, want, what + " sharded") > 1:
                n_multi += 1
    assert n_multi >= 2, "the long pulses and the train must be compared on several shards"
    ctx.close()
    sh.close()


@pytest.mark.parametrize("sps", [6, 8, 20])
def test_full_lists_on_short_chunks(native, torch_mod, sps):
    """A train of four tiles per resident wavefront and more, |IQ|^2 floats, int8 and uint8.  Whether lists are still full at chunk ends (pend_flush) rests on
    the library's chunk plan: the ABI has no chunk setting, and nothing on the GPU logs the route.  So the test asserts the
    |IQ|^2 call's plan (adsb_plan_chunks for this device's resident wavefronts, and the k_detect grid the call used) and,
    under that plan, that the pending-list model of burst_paths -- checked against the emulator's route log in
    test_sim_burst_paths.test_full_lists_at_every_grid -- has full lists at chunk ends.  The 8-bit formats run one
    wavefront per workgroup: other chunks, the same train."""
    ctx = native.Context(sps * 1e6, 0.01)
    ctx.process_mag2(np.zeros(1 << 20, np.float32))
    resident = torch_mod.cuda.get_device_properties(0).multi_processor_count * ctx.stats()["blocks_per_cu"] * 4
    # four tiles per resident wavefront and more: chunks of several tiles, so that lists carry from tile to tile
    i, q = B.preamble_train(sps, n_tiles=max(600, 4 * resident + 40), seed=2)
    for fmt, scale in (("mag2", None), ("sc8", 1.0 / 128.0), ("cu8", 1.0 / 255.0)):
        f = E.FORMATS[fmt][0]
        data, x = E.encode(fmt, i, q, scale)
        thr = B.threshold(fmt, scale)
        ctx.set_threshold(thr)
        if scale is not None:
            ctx.set_format_scale(f, scale)
        want, cands = C.canonical(x, sps, thr, want_cands=True)
        assert len(B.full_list_centres(cands, sps)) > 100
        assert_recs_equal(ctx.process_format(f, data), want, "%s train %d Msps" % (fmt, sps))
        if fmt == "mag2":
            units, chunk = native.plan_chunks(len(x) - (8 * sps - 1), resident)
            assert ctx.stats()["detect_grid"] == (units + 3) // 4 and units > 4, (units, chunk)
            assert len(B.pending_routes(cands, sps, chunk)[1]) > 0, "no list is full at a chunk end under this plan"
    ctx.close()


def _blocks(g, sched, paired):
    from gr_adsb_amd import blocks, grshim
    fr = blocks.framer(g.fs, g.thr)
    dm = blocks.demod(g.fs, framer=fr if paired else None)
    dm.start_timestamp = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tags, msgs = grshim.drive(fr, dm, g.x, None if sched == "single" else g.sched(sched))
    assert np.array_equal(np.array([t.offset for t in tags], dtype=np.int64), g.get(sched, "tag_offsets"))
    snr = np.array([t.value[1] for t in tags], dtype=np.float32)
    assert np.array_equal(snr.view(np.uint32), g.get(sched, "tag_snr_bits"))
    offs = np.array([int(round(m[0]["timestamp"] * g.fs)) for _, m in msgs], dtype=np.int64)
    assert np.array_equal(offs, g.get(sched, "pdu_offsets"))
    assert np.array_equal(np.array([m[1] for _, m in msgs], dtype=np.uint8).reshape(-1, 112), g.pdu_bits(sched))
    psnr = np.array([m[0]["snr"] for _, m in msgs], dtype=np.float32)
    assert np.array_equal(psnr.view(np.uint32), g.get(sched, "pdu_snr_bits"))
    assert fr.prev_eob_idx == int(g.get(sched, "final_prev_eob"))


@pytest.mark.parametrize("name", path_golden_names())
def test_dropin_blocks_match_path_fixtures(native, name):
    g = Golden(name)
    for sched in schedules_of(name):
        for paired in (False, True):
            _blocks(g, sched, paired)
    ctx = native.Context(g.fs, g.thr, flags=native.FLAG_CONFIDENCE)
    recs = ctx.process_mag2(g.x)
    dem = (recs["flags"] & 1) != 0
    assert np.array_equal(recs["offset"], g.get("single", "tag_offsets"))
    assert np.array_equal(unpack(recs["bits"][dem]), g.pdu_bits("single"))
    assert np.array_equal(native.confidence_db(ctx.last_confidence()[dem]).view(np.uint32), g.get("single", "pdu_conf_bits"))
    ctx.close()


def _demod_work(ctx, x, nitems_read, tags, fill=0xAB):
    """adsb_demod_work with every output byte set to `fill` first (Context.demod_work hands it zeroed arrays): returns
    (bits[ntags, 112], ok[ntags] flag bytes, ratio[ntags, 112])"""
    import ctypes
    x = np.ascontiguousarray(x, dtype=np.float32)
    tags = np.ascontiguousarray(tags, dtype=np.int64)
    nt = len(tags)
    bits = np.full((nt, 112), fill, np.uint8)
    ok = np.full(nt, fill, np.uint8)
    ratio = np.full((nt, 112 * 4), fill, np.uint8).view(np.float32)
    rc = ctx.lib.adsb_demod_work(ctx._h, ctypes.c_void_p(x.ctypes.data), len(x), int(nitems_read), ctypes.c_void_p(tags.ctypes.data),
                                 nt, ctypes.c_void_p(bits.ctypes.data), ctypes.c_void_p(ok.ctypes.data),
                                 ctypes.c_void_p(ratio.ctypes.data))
    assert rc == 0, rc
    return bits, ok, ratio


@pytest.mark.parametrize("fec", [False, True])
@pytest.mark.parametrize("sps", [2, 4, 8, 6])
def test_demod_work_slice_edges(native, sps, fec):
    """adsb_demod_work (k_slice, + k_fec_slices with ADSB_FLAG_FEC_CONSERVATIVE) against demod.py:57-136: the last sliced
    and first dropped tag, tags in front of the chunk, duplicates, unsorted, 9000 tags (past the grid's 2048 x 4
    wavefronts), ratios 0/0, x/0, inf/inf, subnormal/normal as float32 bits; the rows of dropped tags come back zero
    although the call before left bits in the same rows of the context's scratch and the host arrays start non-zero"""
    ctx = native.Context(sps * 1e6, 0.01, flags=native.FLAG_FEC_CONSERVATIVE if fec else 0)
    for name, x, tags in B.slice_cases(sps):
        nr = 1000
        # first the same number of tags, all on a burst that is sliced (non-zero bits): the context's device-visible
        # scratch for this call then holds bits in every row, and a dropped row of the next call must be zeroed by k_slice
        dirty, _, _ = _demod_work(ctx, x, nr, np.full(len(tags), nr + 50, np.int64))
        assert dirty.any()
        bits, okb, ratio = _demod_work(ctx, x, nr, tags + nr)
        ok = okb != 0
        sel, wbits, wratio, _ = O.demod_call(x, sps, nr, tags + nr)
        assert np.array_equal(np.flatnonzero(ok), sel), name
        assert not np.any(bits[~ok]) and not np.any(okb[~ok]), name
        assert not np.any(ratio[~ok].view(np.uint32)), name           # adsb_demod_work: zero ratios for dropped tags
        assert np.array_equal(ratio[ok].view(np.uint32), wratio.view(np.uint32)), name
        if not fec:
            assert np.array_equal(bits[ok], wbits), name
            assert np.array_equal(O.mode_s_parity(wbits)["flags"] & 0xE0, okb[ok] & 0xE0), name
        else:
            for k, row in zip(np.flatnonzero(ok), wbits):
                fl, rep, _, _ = native.mode_s_fec(O.pack_bits(row[None])[0])
                assert np.array_equal(native.demod_flags(okb[k:k + 1])[0] & 0xC0E0, fl & 0xC0E0), name
                assert np.array_equal(O.pack_bits(bits[k:k + 1])[0], rep), name
        if name == "edges":
            assert list(ok[:2]) == [True, False]
    ctx.close()
