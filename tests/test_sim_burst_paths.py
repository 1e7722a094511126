"""The burst-record routes of tests/burst_paths.py on the CPU SIMT emulator (the shipped adsb_device.h compiled for the
host, with ADSB_ROUTE logging which site sliced which burst): every k_detect instance -- every format at its default scale,
the integer formats also at a power-of-two scale (int8 / uint8: the dot-product instances) and at a scale that is not one
-- bit for bit against the C oracle on the oracle's |IQ|^2 of the same bytes, with the route log showing that the routes
each stream is built for made records the gate keeps.  Plus chunked framer calls and k_slice, sharded runs whose borders
cut a long run and a dense train, k_confidence's ratios, k_detect's virtual rise, and k_slice at its edges."""
import warnings

import numpy as np
import pytest

import burst_paths as B
import edge_cases as E
import simlib
from helpers import Golden, assert_recs_equal, path_golden_names, schedules_of, unpack
from oracle import adsb_oracle as O
from oracle import c_oracle as C

# (format, scale label, scale): the library default, a power of two and a scale that is not one
INSTANCES = [("fc32", "-", None), ("mag2", "-", None),
             ("sc16", "default", 1.0 / 32768.0), ("sc16", "2^-10", 2.0 ** -10), ("sc16", "3/1024", 3.0 / 1024.0),
             ("sc8", "default", 1.0 / 128.0), ("sc8", "2^-4", 2.0 ** -4), ("sc8", "3/256", 3.0 / 256.0),
             ("cu8", "default", 1.0 / 255.0), ("cu8", "2^-7", 2.0 ** -7), ("cu8", "3/256", 3.0 / 256.0)]
GRIDS = (1, 2, 6)


def test_generator_geometry_is_the_kernels():
    tile, fwd, _ = simlib.kernel_geometry()
    assert (B.TILE, B.WWIN) == (tile, tile + fwd)


def _kept_by(got, log, routes):
    return {r: int(np.isin(got["offset"], log[r]).sum()) for r in routes}


def _check(mode, data, x, sps, thr, scale, what, routes, grid_max, conf=True):
    want = C.canonical(x, sps, thr)
    simlib.route_reset()
    cap = len(x) // 2 + 16
    with simlib.confidence_out(cap) as ratio:
        got, so = simlib.sim_canonical(mode, data, sps * 1e6, thr, scale=1.0 if scale is None else scale, grid_max=grid_max)
    log = simlib.route_offsets()
    assert so.overflow == 0
    assert_recs_equal(got, want, what)
    kept = _kept_by(got, log, routes)
    assert all(kept.values()), "%s: no kept record from routes %r (log %r)" % (what, kept, {k: len(v) for k, v in log.items()})
    if conf:
        # k_confidence: float32 b1 / b0 of demod.py:97-101 for every record with a PDU, as bit patterns; other rows untouched
        dem = (got["flags"] & 1) != 0
        _, _, r, _ = O.demod_call(x, sps, 0, got["offset"][dem])
        assert np.array_equal(ratio[:len(got)][dem].view(np.uint32), r.view(np.uint32)), what + ": confidence ratios"
        assert np.all(ratio[:len(got)][~dem].view(np.uint32) == 0xFFFFFFFF), what + ": rows without a PDU"
    return got, log


@pytest.mark.parametrize("sps", B.RATES)
@pytest.mark.parametrize("fmt,label,scale", INSTANCES)
def test_routes_every_instance(fmt, label, scale, sps):
    mode = E.FORMATS[fmt][0]
    thr = B.threshold(fmt, scale)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, (name, i, q, routes) in enumerate(B.streams(sps)):
            data, x = E.encode(fmt, i, q, scale)
            if name == "long pulses":
                _, _, cases = B.long_pulses(sps)
                mc = B.matched_centres(x, sps, thr)
                assert all(p in mc for _, p, _ in cases), "premise: every long-pulse centre matches"
            if name == "preamble train" and sps >= 6:
                _, cands = C.canonical(x, sps, thr, want_cands=True)
                assert len(B.full_list_centres(cands, sps)) > 0, "premise: a pending list overflows"
            if name == "chained preambles":                      # premise: the bursts past the gates arrive at full lists
                _, _, kept = B.chained_preambles(sps)
                _, cands = C.canonical(x, sps, thr, want_cands=True)
                assert np.array_equal(B.full_list_centres(cands, sps), kept)
            got, log = _check(mode, data, x, sps, thr, scale, "%s %s %d Msps: %s" % (fmt, label, sps, name), routes,
                              GRIDS[k % len(GRIDS)], conf=(label in ("-", "default")))
            if name == "long pulses":                            # every long-pulse centre came out of k_longrun
                longs = [p for _, p, r in cases if r == "long"]
                assert np.isin(longs, np.r_[log["long_fast"], log["long_clipped"]]).all()
            if name == "chained preambles":
                assert np.isin(kept, got["offset"]).all() and np.isin(kept, log["pend_full"]).all()


@pytest.mark.parametrize("sps", B.RATES)
def test_signed_zero_runs(sps):
    """thr 0.0 on |IQ|^2: runs of +0.0 / -0.0 / small values with long-pulse bursts -- zero medians, +0/-0 bit pairs"""
    x, ps = B.signed_zero_runs(sps)
    for g in GRIDS:
        got, log = _check(1, x, x, sps, np.float32(0.0), None, "signed zeros %d Msps grid %d" % (sps, g), {"long_fast"}, g)
        assert np.isin(ps, got["offset"]).all()
        assert np.any(got["median"] == 0) and not np.any(np.signbit(got["median"][got["median"] == 0]))


@pytest.mark.parametrize("sps", [6, 8, 20])
def test_full_lists_at_every_grid(sps):
    """the train with 1, 2 and 6 resident workgroups: the full-list and pend_flush routes at every chunk plan, |IQ|^2 floats
    and complex64; among the bursts pend_flush finishes are some whose list was still full at the chunk's end
    (burst_paths.pending_routes under the emulator's chunk plan, adsb_plan.h)"""
    from gr_adsb_amd import _native
    i, q = B.preamble_train(sps, seed=1)
    for fmt in ("mag2", "fc32"):
        data, x = E.encode(fmt, i, q, None)
        thr = B.threshold(fmt, None)
        _, cands = C.canonical(x, sps, thr, want_cands=True)
        for g in GRIDS:
            _, log = _check(E.FORMATS[fmt][0], data, x, sps, thr, None, "%s train %d Msps grid %d" % (fmt, sps, g),
                            {"pend_full", "flush"}, g, conf=False)
            _, chunk = _native.plan_chunks(len(x) - (8 * sps - 1), g * 4)
            _, flushed_full = B.pending_routes(cands, sps, chunk)
            assert len(flushed_full) and np.isin(flushed_full, log["flush"]).any()


def _stream_and_schedules(sps):
    """a long-pulse stream and a train back to back (|IQ|^2), with the fixed-2048 and a random 1-3000 schedule of the
    fixtures, and calls of 8192 (long enough for runs that leave the LDS window to fall inside one call)"""
    i1, q1, _ = B.long_pulses(sps)
    i2, q2 = B.preamble_train(sps, n_tiles=16)
    _, x = E.encode("mag2", np.r_[i1, i2], np.r_[q1, q2], None)
    n = len(x)
    rng = np.random.default_rng(sps)
    rand, rem = [], n
    while rem > 0:
        c = int(min(rem, rng.integers(1, 3001)))
        rand.append(c)
        rem -= c
    fixed = lambda c: [c] * (n // c) + ([n % c] if n % c else [])          # noqa: E731
    return x, {"fixed2048": fixed(2048), "fixed8192": fixed(8192), "random": rand}


@pytest.mark.parametrize("sps", [2, 8, 20, 12])
def test_chunked_framer_and_demod(sps):
    """framer.work() calls on a schedule (adsb_plan.h's framer plan, k_detect / k_longrun per call) and the stand-alone
    demod's k_slice per chunk, against the NumPy oracle's run_stream on the same schedule"""
    x, scheds = _stream_and_schedules(sps)
    thr = B.threshold("mag2", None)
    H = 8 * sps
    buf = np.concatenate([np.zeros(H - 1, np.float32), x])
    n_long = 0
    for sname, sched in scheds.items():
        with np.errstate(all="ignore"):
            o = O.run_stream(x, sps * 1e6, thr, sched)
        for g in (1, 6):
            fr = simlib.SimFramer(sps * 1e6, thr, grid_max=g)
            pos, outs = 0, []
            simlib.route_reset()
            for N in sched:
                outs.append(fr.work(buf[pos:pos + N + H - 1], N, pos)[0])
                pos += N
            recs = np.concatenate(outs)
            assert np.array_equal(recs["offset"], o["tag_offsets"]), sname
            assert np.array_equal(recs["peak"].view(np.uint32), o["tag_peak"].view(np.uint32)), sname
            assert np.array_equal(recs["median"].view(np.uint32), o["tag_median"].view(np.uint32)), sname
            assert fr.prev_eob.value == o["final_prev_eob"]
            log = simlib.route_offsets()
            n_long += len(log["long_fast"]) + len(log["long_clipped"])
        pos, offs, bits, ratio = 0, [], [], []
        t = o["tag_offsets"]
        for N in sched:
            inside = np.flatnonzero((t >= pos) & (t < pos + N))
            if len(inside):
                b, ok, r = simlib.sim_slice(x[pos:pos + N], t[inside] - pos, sps)
                sel = ok.astype(bool)
                offs.append(t[inside][sel]); bits.append(unpack(b[sel])); ratio.append(r[sel])
            pos += N
        assert np.array_equal(np.concatenate(offs), o["pdu_offsets"]), sname
        assert np.array_equal(np.concatenate(bits), o["pdu_bits"]), sname
        assert np.array_equal(np.concatenate(ratio).view(np.uint32), o["pdu_ratio"].view(np.uint32)), sname
    assert n_long > 0, "no framer call finished a run through k_longrun"


def shard_plans(n, borders, sps, max_run=8 * 1024):
    """frontend.shard_plan's halos around owner borders of our choosing (max_run: the longest run a shard follows)"""
    from gr_adsb_amd.frontend import NOISE_BACK
    edges = [0] + list(borders) + [n]
    plans = []
    for a, b in zip(edges[:-1], edges[1:]):
        lo = max(0, a - (NOISE_BACK + 8 * sps + 4))
        lo -= lo % 4
        plans.append(dict(own_lo=a, own_hi=b, lo=lo, hi=min(n, b + max_run + 121 * sps)))
    return plans


@pytest.mark.parametrize("sps", [4, 8, 20])
@pytest.mark.parametrize("mode", [0, 1])
def test_shards_cut_long_runs_and_trains(mode, sps):
    """overlapped shards whose owner borders lie inside a run over five tiles, inside a run that leaves the LDS window by
    one sample and inside a dense train; stitched and gated they equal one canonical call"""
    i1, q1, cases = B.long_pulses(sps)
    i2, q2 = B.preamble_train(sps, n_tiles=16)
    fmt = "fc32" if mode == 0 else "mag2"
    data, x = E.encode(fmt, np.r_[i1, i2], np.r_[q1, q2], None)
    n = len(x)
    thr = B.threshold(fmt, None)
    p5 = [p for name, p, _ in cases if name == "run over 5 tiles"][0]
    p1 = [p for name, p, _ in cases if name.endswith("run=WWIN-r+0")][0]
    borders = sorted([p1 - 3, p5 + 17, len(i1) + 5 * B.TILE + 333])
    want, cands = C.canonical(x, sps, thr, want_cands=True)
    parts = []
    simlib.route_reset()
    for pl in shard_plans(n, borders, sps):
        r, so = simlib.sim_shard(mode, data[pl["lo"]:pl["hi"]], pl["lo"], pl["own_lo"], pl["own_hi"], n, sps * 1e6, thr, grid_max=2)
        assert (so.flags & 4) == 0
        parts.append(r)
    c = np.concatenate(parts)
    assert np.array_equal(c["offset"], cands)
    assert_recs_equal(c[O.resolve_candidates(c["offset"], sps)], want, "stitched shards")
    log = simlib.route_offsets()
    assert np.isin([p1, p5], log["long_fast"]).all()
    if sps >= 6:
        assert len(log["pend_full"]) and len(log["flush"])


@pytest.mark.parametrize("sps,p", [(2, 20), (2, 60), (4, 50), (8, 5), (8, 30), (6, 13)])
def test_virtual_rise_through_the_argument_block(sps, p):
    """k_detect's virtual rise: unit 0 of a call whose scan starts in the zero history (scan_lo < 0) at thr 0.0, after a
    previous sample below it -- a framer state no entry point creates (burst_paths' docstring), so it is driven through
    the kernel's argument block directly (simlib.sim_run, prev_in0 = -1).  The run that starts at in0[0] is finished by
    k_longrun; its centre lies within 100 samples of in0[0], so burst_finish clips the noise window at in0_base.  Against
    the NumPy oracle's framer_call with the same state."""
    H = 8 * sps
    half = sps // 2
    n = 6 * B.TILE
    rng = np.random.default_rng(p + sps)
    x = -(np.float32(0.25) + rng.random(n, dtype=np.float32))
    P = p + H - 1                                               # the centre as an in0 index
    fall = 2 * P - (H - 1) + 1                                  # local index of the run's fall: (0 + fall_in0) // 2 == P
    x[:fall] = (rng.random(fall) * 0.01).astype(np.float32)
    x[:fall:11] = np.float32(-0.0)
    for c in (0, 2, 7, 9):
        x[p + c * half:p + c * half + half] = np.float32(1.0)
    for c in (1, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15):
        if p + c * half + half <= fall:
            x[p + c * half:p + c * half + half] = np.float32(0.0)
    for k, b in enumerate(B._frame(rng)):
        j1 = p + 8 * sps + k * sps
        x[(j1 if b else j1 + half):(j1 if b else j1 + half) + half] = np.float32(0.75)
    x[fall] = np.float32(-0.5)
    assert P < 100                                             # the noise window in0[max(0, P - 100):P] is clipped
    st = O.FramerState()
    st.prev_in0 = np.float32(-1.0)
    buf = np.concatenate([np.zeros(H - 1, np.float32), x])
    with np.errstate(all="ignore"):
        fr = O.framer_call(buf, n, sps, np.float32(0.0), st, 0)
    assert len(fr["tag_offsets"]) and fr["tag_offsets"][0] == p
    sel, bits, _, _ = O.demod_call(x, sps, 0, fr["tag_offsets"])
    simlib.route_reset()
    got, so = simlib.sim_run(1, x, sps, 0.0, in0_base=-(H - 1), scan_lo=-(H - 1), scan_hi=n - (H - 1), fall_hi=n - (H - 1),
                             dem_hi=n, prev_in0=-1.0)
    assert np.array_equal(got["offset"], fr["tag_offsets"])
    assert np.array_equal(got["peak"].view(np.uint32), fr["peak"].view(np.uint32))
    assert np.array_equal(got["median"].view(np.uint32), fr["median"].view(np.uint32))
    dem = (got["flags"] & 1) != 0
    assert np.array_equal(np.flatnonzero(dem), sel)
    assert np.array_equal(unpack(got["bits"][dem]), bits)
    assert p in simlib.route_offsets()["long_clipped"]


@pytest.mark.parametrize("sps", [2, 4, 8, 6])
def test_slice_edges(sps):
    """k_slice against demod.py:57-136 (O.demod_call): the last sliced and first dropped tag, tags in front of the chunk,
    duplicates, unsorted, more tags than wavefronts, ratios 0/0, x/0, inf/inf, subnormal/normal as float32 bits; rows
    of dropped tags come back zeroed (bits, flags), their ratios untouched"""
    for name, x, tags in B.slice_cases(sps):
        bits, ok, ratio = simlib.sim_slice(x, tags, sps, fill=0xAB)
        sel, wbits, wratio, _ = O.demod_call(x, sps, 0, tags)
        dem = (ok & 1) != 0
        assert np.array_equal(np.flatnonzero(dem), sel), name
        assert np.array_equal(unpack(bits[dem]), wbits), name
        assert np.array_equal(ratio[dem].view(np.uint32), wratio.view(np.uint32)), name
        assert not np.any(bits[~dem]) and not np.any(ok[~dem]), name
        assert np.all(ratio[~dem].view(np.uint32) == 0xABABABAB), name
        assert np.array_equal(O.mode_s_parity(wbits)["flags"] & 0xE0, ok[dem] & 0xE0), name
        if name == "edges":
            assert list(dem[:2]) == [True, False]


@pytest.mark.parametrize("name", path_golden_names())
def test_emulated_calls_match_path_fixtures(name):
    """the reference fixtures (tools/make_golden_paths.py): the canonical call, and framer calls + k_slice per chunk on the
    stored schedules"""
    g = Golden(name)
    H = 8 * g.sps
    got, _ = simlib.sim_canonical(1, g.x, g.fs, np.float32(g.thr))
    dem = (got["flags"] & 1) != 0
    assert np.array_equal(got["offset"], g.get("single", "tag_offsets"))
    assert np.array_equal(unpack(got["bits"][dem]), g.pdu_bits("single"))
    buf = np.concatenate([np.zeros(H - 1, np.float32), g.x])
    for sched in schedules_of(name):
        fr = simlib.SimFramer(g.fs, np.float32(g.thr), grid_max=2)
        pos, outs, offs, bits = 0, [], [], []
        for N in g.sched(sched):
            outs.append(fr.work(buf[pos:pos + N + H - 1], N, pos)[0])
            pos += N
        t = np.concatenate(outs)["offset"]
        assert np.array_equal(t, g.get(sched, "tag_offsets")), sched
        pos = 0
        for N in g.sched(sched):
            inside = np.flatnonzero((t >= pos) & (t < pos + N))
            if len(inside):
                b, ok, _ = simlib.sim_slice(g.x[pos:pos + N], t[inside] - pos, g.sps)
                offs.append(t[inside][ok.astype(bool)]); bits.append(unpack(b[ok.astype(bool)]))
            pos += N
        assert np.array_equal(np.concatenate(offs) if offs else np.zeros(0, np.int64), g.get(sched, "pdu_offsets")), sched
        if offs:
            assert np.array_equal(np.concatenate(bits), g.pdu_bits(sched)), sched
