"""Receiver streams carried across batch calls (adsb_process_stream_batch*: k_stream_stage, k_batch, k_batch_pack,
k_stream_save) on the CPU SIMT emulator (tests/sim/stream_driver.cpp), against the reference's single-call vectors and against
the ordinary pass over the whole stream (simlib.sim_canonical); the plan's arithmetic; the new kernels' build facts; the ABI
of the new entry points.  Every comparison of records is byte for byte."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import simlib
from gr_adsb_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
STREAM_SO = os.path.join(SIM_DIR, "libadsb_stream_sim.so")
ROOT = os.path.dirname(HERE)
_DT = {0: np.complex64, 1: np.float32, 2: np.int16, 3: np.int8, 4: np.uint8}
_PER = {0: 1, 1: 1, 2: 2, 3: 2, 4: 2}          # array elements per sample
FRESH_EOB = -(1 << 61)


def B_of(sps):
    return 100 + 8 * sps + 4


def F_of(sps):
    return 256 + 121 * sps


def carry_start(pos, sps):
    """the first stream sample the next call's buffer holds: B + F in front of pos, down to a multiple of 8 samples"""
    return max(0, (pos - B_of(sps) - F_of(sps)) // 8 * 8)


def _lib():
    csrc = os.path.join(ROOT, "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, "stream_driver.cpp"), os.path.join(SIM_DIR, "hipsim.h"), os.path.join(csrc, "adsb_device.h"),
            os.path.join(csrc, "adsb_plan.h")]
    if not (os.path.exists(STREAM_SO) and all(os.path.getmtime(STREAM_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", STREAM_SO])
    lib = ctypes.CDLL(STREAM_SO)
    lib.stream_open.restype = ctypes.c_void_p
    lib.stream_carry.restype = ctypes.c_longlong
    lib.stream_carry_max_samples.restype = ctypes.c_longlong
    return lib


class Streams:
    """a set of emulated streams of one format and rate"""

    def __init__(self, mode, sps, n_streams, scale=1.0, long_aware=False):
        self.lib = _lib()
        self.mode, self.sps, self.n = mode, sps, n_streams
        self.h = ctypes.c_void_p(self.lib.stream_open(ctypes.c_int(mode), ctypes.c_int(sps), ctypes.c_int(n_streams),
                                                      ctypes.c_float(scale), ctypes.c_int(1 if long_aware else 0)))
        assert self.h

    def close(self):
        self.lib.stream_close(self.h)

    def set_base(self, sid, base):
        return self.lib.stream_set_base(self.h, ctypes.c_int(sid), ctypes.c_longlong(base))

    def state(self, sid):
        """(pos, eob, overlong)"""
        p, e, o = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        assert self.lib.stream_state(self.h, ctypes.c_int(sid), ctypes.byref(p), ctypes.byref(e), ctypes.byref(o)) == 0
        return p.value, e.value, o.value

    def carry(self, sid):
        cap = int(self.lib.stream_carry_max_samples(ctypes.c_int(self.sps))) * 8
        buf = np.zeros(cap, dtype=np.uint8)
        nb = self.lib.stream_carry(self.h, ctypes.c_int(sid), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(cap))
        assert nb >= 0
        return buf[:nb].view(_DT[self.mode])

    def push(self, ids, arrays, thrs, end=None, rec_cap=0, device_entry=False):
        """-> (list of per-item record arrays, kept[], summary flags[])"""
        c = ctypes
        k = len(ids)
        per = _PER[self.mode]
        arrays = [np.ascontiguousarray(a, dtype=_DT[self.mode]) for a in arrays]
        ptrs = (c.c_void_p * k)(*[a.ctypes.data for a in arrays])
        ns = np.array([len(a) // per for a in arrays], dtype=np.int64)
        idv = np.asarray(ids, dtype=np.int32)
        endv = np.zeros(k, dtype=np.int32) if end is None else np.asarray(end, dtype=np.int32)
        th = np.asarray(thrs, dtype=np.float32)
        assert len(th) == k and len(endv) == k
        cap = int(ns.sum()) // 2 + 700 * k + 64
        out = np.zeros(cap, dtype=simlib.REC_DTYPE)
        first = np.full(k + 1, -9, dtype=np.int32)
        kept = np.full(k, -9, dtype=np.int32)
        fl = np.zeros(k, dtype=np.uint32)
        rc = self.lib.stream_push(self.h, c.c_int(k), idv.ctypes.data_as(c.c_void_p), ptrs, ns.ctypes.data_as(c.c_void_p),
                                  endv.ctypes.data_as(c.c_void_p), th.ctypes.data_as(c.c_void_p), c.c_int(rec_cap),
                                  c.c_int(1 if device_entry else 0), out.ctypes.data_as(c.c_void_p), c.c_int(cap),
                                  first.ctypes.data_as(c.c_void_p), kept.ctypes.data_as(c.c_void_p), fl.ctypes.data_as(c.c_void_p))
        assert rc >= 0, rc
        assert first[0] == 0 and first[-1] == rc and np.all(np.diff(first) >= 0), first
        return [out[first[i]:first[i + 1]].copy() for i in range(k)], kept, fl


def cuts_fixed(n, step):
    return [min(step, n - a) for a in range(0, n, step)]


def cuts_random(n, hi, seed, specials=(0, 1, 3, 0, 255)):
    """chunk lengths 0..hi that sum to n; `specials` are mixed in first (zero, one, odd and short lengths)"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    for s in specials:
        a = int(rng.integers(0, hi + 1))
        for v in (a, s):
            v = min(v, left)
            out.append(v)
            left -= v
    while left > 0:
        v = min(int(rng.integers(0, hi + 1)), left)
        out.append(v)
        left -= v
    return out


def run_streams(S, sources, cuts, thrs, device_entry=False, check_carry=False, rec_cap=0):
    """sources[i]: the whole stream i in the format's layout; cuts[i]: its chunk lengths (samples).  One call per round pushes
    the next chunk of every stream that still has one; a last call ends them all.  -> per stream: concatenated records"""
    per = _PER[S.mode]
    k = len(sources)
    pos = [0] * k
    nxt = [0] * k
    got = [[] for _ in range(k)]
    while any(nxt[i] < len(cuts[i]) for i in range(k)):
        ids = [i for i in range(k) if nxt[i] < len(cuts[i])]
        arrays = []
        for i in ids:
            n = cuts[i][nxt[i]]
            arrays.append(sources[i][pos[i] * per:(pos[i] + n) * per])
            pos[i] += n
            nxt[i] += 1
        recs, kept, _ = S.push(ids, arrays, [thrs[i] for i in ids], device_entry=device_entry, rec_cap=rec_cap)
        assert np.all(kept >= 0)
        for j, i in enumerate(ids):
            got[i].append(recs[j])
            assert S.state(i)[0] == pos[i]
            if check_carry:
                want = sources[i][carry_start(pos[i], S.sps) * per:pos[i] * per]
                assert S.carry(i).tobytes() == np.ascontiguousarray(want).tobytes(), (i, pos[i])
    empty = np.zeros(0, dtype=_DT[S.mode])
    recs, kept, _ = S.push(list(range(k)), [empty] * k, thrs, end=[1] * k, device_entry=device_entry, rec_cap=rec_cap)
    assert np.all(kept >= 0)
    for i in range(k):
        assert pos[i] * per == len(sources[i])
        got[i].append(recs[i])
        assert S.state(i)[:2] == (0, FRESH_EOB)
    return [np.concatenate(g) for g in got]


# ---- 1. the reference's single-call vectors as streams, several per call at different phases -------------------------
@pytest.mark.parametrize("name", helpers.golden_names())
def test_goldens_as_streams_under_schedules(name):
    g = helpers.Golden(name)
    n = len(g.x)
    x = np.asarray(g.x, dtype=np.float32)
    F = F_of(g.sps)
    cuts = [cuts_fixed(n, 4096), g.sched("random"), cuts_random(n, 3000, seed=11), cuts_random(n, 70000, seed=12),
            [F - 1, 1, F, 5] + cuts_fixed(n - 2 * F - 5, 8192)]
    for c in cuts:
        assert sum(c) == n
    assert 0 in cuts[2] and 1 in cuts[2] and any(v % 2 for v in cuts[2]) and min(cuts[4]) < F
    S = Streams(1, g.sps, len(cuts))
    try:
        got = run_streams(S, [x] * len(cuts), cuts, [g.thr] * len(cuts), check_carry=True)
        for i, r in enumerate(got):
            helpers.assert_recs_match_golden(r, g, "single")
            assert S.state(i)[2] == 0, "overlong pulses in stream %d" % i      # the condition under which equality is claimed
    finally:
        S.close()


@pytest.mark.parametrize("name,mode", [("L2msps_df17", 3), ("R6msps", 3), ("L2msps_df17", 0)])
def test_large_goldens_as_streams(name, mode):
    g = helpers.Golden(name)
    n = len(g.x)
    src = g.iq8 if mode == 3 else g.iq
    cuts = [cuts_random(n, 70000, seed=5), cuts_fixed(n, 65536 + 3)]
    S = Streams(mode, g.sps, 2, scale=float(g.scale) if mode == 3 else 1.0)
    try:
        got = run_streams(S, [src, src], cuts, [g.thr, g.thr], device_entry=(mode == 0))
        for i, r in enumerate(got):
            helpers.assert_recs_match_golden(r, g, "single")
            assert S.state(i)[2] == 0
    finally:
        S.close()


# ---- 2. the integer formats against the ordinary pass over the whole stream ------------------------------------------
def _format_stream(mode, sps):
    rep = sps // 2
    if mode == 2:
        z = np.load(os.path.join(helpers.GOLDEN_DIR, "g2msps_df17.npz"))
        pairs = z["iq16"].reshape(-1, 2)[2000:2000 + 30000]
        return np.repeat(pairs, rep, axis=0).reshape(-1), float(z["threshold"]), 2.0 / 32767.0
    a = helpers.rise_storm_iq8(24000 * rep, seed=7, offset_binary=(mode == 4), half=rep)
    return a, 0.01, (1.0 / 128.0 if mode == 3 else 1.0 / 255.0)


@pytest.mark.parametrize("device_entry", [False, True])
@pytest.mark.parametrize("sps", [2, 8])
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_formats_equal_the_ordinary_pass_over_the_whole_stream(mode, sps, device_entry):
    src, thr, scale = _format_stream(mode, sps)
    n = len(src) // 2
    if mode == 4:
        # the fresh-stream rule: bursts inside the first 8 * sps samples, and nothing (no zero BYTES, which offset binary
        # does not convert to 0) in front of the stream's first sample
        assert np.any(src[:16 * sps] > 140)
    cuts = [cuts_random(n, 3000, seed=21), cuts_fixed(n, 4099), [n]]
    S = Streams(mode, sps, len(cuts), scale=scale)
    try:
        got = run_streams(S, [src] * len(cuts), cuts, [thr] * len(cuts), device_entry=device_entry, check_carry=True,
                          rec_cap=2048)
        want, _ = simlib.sim_canonical(mode, src, sps * 1e6, thr, scale=scale)
        assert (want["flags"] & 1).sum() > 10
        for i, r in enumerate(got):
            assert r.tobytes() == want.tobytes(), "stream %d" % i
            assert S.state(i)[2] == 0
    finally:
        S.close()


# ---- 3. a pulse longer than the carry --------------------------------------------------------------------------------
def test_an_overlong_pulse_across_a_seam_is_dropped_and_counted():
    g = helpers.Golden("Qpaths_8msps")
    x = np.asarray(g.x, dtype=np.float32)
    n = len(x)
    hi = x >= g.thr
    # the longest run of samples above the threshold: a pulse longer than the look-ahead F
    edges = np.flatnonzero(np.diff(np.concatenate(([0], hi.view(np.int8), [0]))))
    runs = edges.reshape(-1, 2)
    a, b = runs[np.argmax(runs[:, 1] - runs[:, 0])]
    F = F_of(g.sps)
    assert b - a > F + 16
    cut = int(a) + F + 8                      # the call that owns the pulse's rise ends while the pulse is still high
    S = Streams(1, g.sps, 1)
    try:
        got = run_streams(S, [x], [[cut, n - cut]], [g.thr])[0]
        assert S.state(0)[2] > 0
        want, _ = simlib.sim_canonical(1, x, g.fs, g.thr)
        have = {r.tobytes() for r in want}
        assert len(got) > 0 and all(r.tobytes() in have for r in got)
    finally:
        S.close()


# ---- 4. one call, mixed items ----------------------------------------------------------------------------------------
def test_fresh_running_ending_and_empty_items_in_one_call():
    g = helpers.Golden("g2msps_df17")
    x = np.asarray(g.x[:60000], dtype=np.float32)
    e = np.zeros(0, dtype=np.float32)
    want, _ = simlib.sim_canonical(1, x, g.fs, g.thr)
    want7, _ = simlib.sim_canonical(1, x, g.fs, g.thr, abs_offset=7000)
    assert len(want) > 20
    S = Streams(1, g.sps, 5)
    try:
        assert S.set_base(3, 7000) == 0
        # call 1: streams 0 and 1 start
        r1, _, _ = S.push([0, 1], [x[:20000], x[:33333]], [g.thr] * 2)
        assert S.set_base(1, 5) != 0                                    # only a fresh stream takes a base
        # call 2: 0 goes on, 1 ends with its last samples, 2 is fresh and ends in the same call, 3 (based) starts, 4 is empty
        r2, kept, _ = S.push([4, 0, 1, 2, 3], [e, x[20000:41001], x[33333:], x, x[:999]], [g.thr] * 5, end=[0, 0, 1, 1, 0])
        assert kept[0] == 0 and len(r2[0]) == 0 and S.state(4)[:2] == (0, FRESH_EOB)
        assert r2[3].tobytes() == want.tobytes()                         # fresh and END at once: the canonical call
        assert np.concatenate([r1[1], r2[2]]).tobytes() == want.tobytes()
        assert S.state(1)[:2] == (0, FRESH_EOB) and S.state(2)[:2] == (0, FRESH_EOB) and S.state(0)[0] == 41001
        # call 3: 1 starts again (offsets restart), 0 and 3 end, 4 ends empty
        r3, kept, _ = S.push([1, 0, 3, 4], [x, x[41001:], x[999:], e], [g.thr] * 4, end=[1, 1, 1, 1])
        assert r3[0].tobytes() == want.tobytes()
        assert np.concatenate([r1[0], r2[1], r3[1]]).tobytes() == want.tobytes()
        assert np.concatenate([r2[4], r3[2]]).tobytes() == want7.tobytes()
        assert len(r3[3]) == 0 and kept[3] == 0
    finally:
        S.close()


def test_a_threshold_applies_to_the_rises_its_call_owns():
    g = helpers.Golden("g2msps_df17")
    x = np.asarray(g.x, dtype=np.float32)
    want, _ = simlib.sim_canonical(1, x, g.fs, g.thr)
    offs = want["offset"]
    k = int(np.argmax(np.diff(offs)[20:-20])) + 20                       # the widest gap between two records, away from the ends
    assert offs[k + 1] - offs[k] > 600
    b = int(offs[k] + offs[k + 1]) // 2                                  # call 1 owns the rises in front of b, call 2 the others
    cut = b + F_of(g.sps)
    deaf = 1e9
    S = Streams(1, g.sps, 2)
    try:
        r1, _, _ = S.push([0, 1], [x[:cut], x[:cut]], [g.thr, deaf])
        r2, _, _ = S.push([0, 1], [x[cut:], x[cut:]], [deaf, g.thr], end=[1, 1])
        assert len(r2[0]) == 0 and r1[0].tobytes() == want[:k + 1].tobytes()
        assert len(r1[1]) == 0 and r2[1].tobytes() == want[k + 1:].tobytes()
    finally:
        S.close()


# ---- 5. the re-trigger gate across seams -----------------------------------------------------------------------------
@pytest.mark.parametrize("long_aware", [False, True])
def test_gate_is_carried_across_seams_inside_chains(long_aware):
    sps = 2
    iq = helpers.preamble_train_iq(1 << 15, spacing=32, sps=sps)         # a centre every 32 symbols: chains inside the 63-symbol gate
    n = len(iq)
    cuts = [cuts_fixed(n, 1000), cuts_random(n, 700, seed=3), cuts_fixed(n, 32 * sps * 7 + 1)]
    ctx = simlib.long_aware_gate() if long_aware else None
    if ctx:
        ctx.__enter__()
    try:
        want, so = simlib.sim_canonical(0, iq, 2e6, 0.01)
    finally:
        if ctx:
            ctx.__exit__()
    assert 0 < len(want) < so.n_rec                                       # the gate did drop centres
    S = Streams(0, sps, len(cuts), long_aware=long_aware)
    try:
        got = run_streams(S, [iq] * len(cuts), cuts, [0.01] * len(cuts), rec_cap=1024)
        for i, r in enumerate(got):
            assert r.tobytes() == want.tobytes(), "stream %d" % i
    finally:
        S.close()


# ---- 6. a forced list overflow ---------------------------------------------------------------------------------------
def test_an_overflowing_item_is_marked_and_disturbs_nobody():
    from gr_adsb_amd import modulator as M
    a = np.ascontiguousarray(M.synth_iq(6000, 2e6, 4000, seed=20))
    b = np.ascontiguousarray(M.synth_iq(9000, 2e6, 4000, seed=22))
    train = helpers.preamble_train_iq(1 << 15)
    S = Streams(0, 2, 3)
    try:
        recs, kept, _ = S.push([0, 1, 2], [a, train, b], [0.01] * 3, end=[1, 1, 1], rec_cap=64)
        assert kept[1] == -1 and len(recs[1]) == 0 and S.state(1)[0] == 0
        for r, src in ((recs[0], a), (recs[2], b)):
            want, _ = simlib.sim_canonical(0, src, 2e6, 0.01)
            assert len(want) > 0 and r.tobytes() == want.tobytes()
    finally:
        S.close()


# ---- 7. the plan ------------------------------------------------------------------------------------------------------
def _plan_py(pos, n, end, base, eob, sps):
    """plan_stream_item restated from the issue's definitions (not from adsb_plan.h)"""
    B, F, H = B_of(sps), F_of(sps), 8 * sps
    origin = max(0, (pos - B - F) // 8 * 8)
    n_buf = pos + n - origin
    stream_len = pos + n if end else 1 << 60
    scan_end = stream_len - (H - 1)
    lo = pos - F
    hi = stream_len if end else pos + n - F
    if lo <= 0:
        lo = -(H - 1)                               # the first owning call owns from the stream's start (origin is 0 then)
    hi = min(hi, scan_end)
    in0_base = -(H - 1) - origin
    run = (n_buf > 0) if end else (pos + n - F > 0)
    return dict(origin=origin + base, n=n_buf, in0_base=in0_base, scan_lo=max(lo - origin, in0_base), scan_hi=hi - origin,
                fall_hi=(scan_end - origin) if end else n_buf, dem_hi=stream_len - origin, end_is_call_end=1 if end else 0,
                prev_eob_stream=eob, gate=1, head_n=0, run=1 if run else 0, stream_origin=origin)


def test_plan_stream_item_against_a_restatement():
    lib = _lib()
    rng = np.random.default_rng(99)
    names = ["origin", "n", "in0_base", "scan_lo", "scan_hi", "fall_hi", "dem_hi", "end_is_call_end", "prev_eob_stream", "gate",
             "head_n", "run", "stream_origin"]
    out = (ctypes.c_longlong * len(names))()
    for k in range(4000):
        sps = int(rng.choice([2, 4, 6, 8, 20, 100]))
        pos = int(rng.choice([0, 0, int(rng.integers(0, 3000)), int(rng.integers(0, 1 << 40))]))
        n = int(rng.choice([0, 1, int(rng.integers(0, 700)), int(rng.integers(0, 1 << 22))]))
        end = bool(rng.integers(0, 2))
        base = int(rng.integers(-5, 1 << 50))
        eob = FRESH_EOB if pos == 0 else base + pos - int(rng.integers(0, 5000))
        lib.stream_plan(ctypes.c_longlong(pos), ctypes.c_longlong(n), ctypes.c_int(end), ctypes.c_longlong(base),
                        ctypes.c_longlong(eob), ctypes.c_int(sps), out)
        want = _plan_py(pos, n, end, base, eob, sps)
        assert {k: int(v) for k, v in zip(names, out)} == want, (pos, n, end, sps)
        # consecutive calls tile the stream: what this one does not own, the next one does
        if not end and want["run"]:
            lib.stream_plan(ctypes.c_longlong(pos + n), ctypes.c_longlong(5), ctypes.c_int(1), ctypes.c_longlong(base),
                            ctypes.c_longlong(eob), ctypes.c_int(sps), out)
            nxt = {k: int(v) for k, v in zip(names, out)}
            assert nxt["scan_lo"] + nxt["stream_origin"] == want["scan_hi"] + want["stream_origin"]
            assert nxt["scan_lo"] >= B_of(sps) or nxt["stream_origin"] == 0          # the noise window and the preamble lie in the buffer


# ---- 8. build facts ---------------------------------------------------------------------------------------------------
def _resources():
    from gr_adsb_amd import build as B
    if not os.path.exists(B.RES):
        pytest.skip("kernel_resources.json is written by the library build")
    with open(B.RES) as f:
        return json.load(f)


def test_stream_kernels_have_no_scratch_no_spills_and_fit_beside_k_detect():
    res = _resources()
    ks = {k: v for k, v in res.items() if "k_stream_" in k}
    assert len(ks) == 2 and any("k_stream_stage" in k for k in ks) and any("k_stream_save" in k for k in ks), sorted(ks)
    for k, v in ks.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v.get("sgpr_spills", 0) == 0, (k, v)
        assert v["lds_bytes_per_block"] == 0                          # nothing to fit beside k_detect's LDS
        assert v["vgprs"] <= 32                                      # the other tail kernels' register room (tests/test_abi.py)
    # the names must not move the counts tests/test_abi.py and tests/test_batch.py hold
    assert not any(t in k for k in ks for t in ("k_detect", "k_order", "k_resolve", "k_count", "k_compact", "k_batch"))


# ---- 9. ABI -----------------------------------------------------------------------------------------------------------
def test_stream_item_layout_and_declared_symbols():
    dt = _native.STREAM_ITEM_DTYPE
    assert dt.itemsize == 32
    assert [dt.fields[n][1] for n in ("data", "n", "stream", "flags", "threshold", "reserved")] == [0, 8, 16, 20, 24, 28]
    assert _native.ABI_VERSION == 5 and _native.STREAM_END == 1
    names = ("adsb_streams_open", "adsb_streams_close", "adsb_stream_set_base", "adsb_stream_state", "adsb_stream_reset",
             "adsb_process_stream_batch", "adsb_process_stream_batch_device")
    hdr = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    for name in names:
        assert name in _native.EXPORTS
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    m = re.search(r"typedef struct adsb_stream_item \{(.*?)\} adsb_stream_item;", hdr, re.S)
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+);", m.group(1), re.M)
    assert fields == [("void", "data"), ("int64_t", "n"), ("int32_t", "stream"), ("uint32_t", "flags"), ("float", "threshold"),
                      ("uint32_t", "reserved")]
    assert re.search(r"#define ADSB_STREAM_END 1u\b", hdr) and re.search(r"#define ADSB_ABI_VERSION 5\b", hdr)
    from gr_adsb_amd import build as B
    if os.path.exists(B.LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], stdout=subprocess.PIPE, text=True).stdout
        for name in names:
            assert (" %s\n" % name) in out, name
