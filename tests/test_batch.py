"""The batch path (adsb_process_batch*: k_batch, one workgroup per independent stream, then k_batch_pack) on the CPU SIMT
emulator (tests/sim/batch_driver.cpp), against the reference's single-call vectors and against the ordinary pass run item by
item (simlib.sim_canonical); the kernels' build facts; the ABI of the new entry points.  Every comparison is byte for byte."""
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
BATCH_SO = os.path.join(SIM_DIR, "libadsb_batch_sim.so")
ROOT = os.path.dirname(HERE)
_DT = {0: np.complex64, 1: np.float32, 2: np.int16, 3: np.int8, 4: np.uint8}


def _lib():
    csrc = os.path.join(ROOT, "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, "batch_driver.cpp"), os.path.join(SIM_DIR, "hipsim.h"), os.path.join(csrc, "adsb_device.h"),
            os.path.join(csrc, "adsb_plan.h")]
    if not (os.path.exists(BATCH_SO) and all(os.path.getmtime(BATCH_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", BATCH_SO])
    lib = ctypes.CDLL(BATCH_SO)
    lib.batch_item_max.restype = ctypes.c_longlong
    return lib


def aligned(a):
    """a copy of `a` that starts on a 64-byte boundary (what a device allocation gives)"""
    a = np.ascontiguousarray(a)
    raw = np.zeros(a.nbytes + 64, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    v = raw[o:o + a.nbytes].view(a.dtype)
    v[...] = a
    return v


def batch_run(mode, sps, arrays, thrs, scale=1.0, rec_cap=0, abs_offsets=None, long_aware=False, host_cap=3):
    """arrays[i]: the item's samples in the format's layout, read IN PLACE (must be 16-byte aligned) ->
    (list of per-item record arrays, item_first, kept[], overflow[])"""
    c = ctypes
    k = len(arrays)
    per = 2 if mode >= 2 else 1
    for a in arrays:
        assert a.dtype == _DT[mode] and a.flags["C_CONTIGUOUS"]
    ptrs = (c.c_void_p * k)(*[a.ctypes.data if len(a) else arrays[0].ctypes.data for a in arrays])
    ns = np.array([len(a) // per for a in arrays], dtype=np.int64)
    offs = np.zeros(k, dtype=np.int64) if abs_offsets is None else np.asarray(abs_offsets, dtype=np.int64)
    th = np.asarray(thrs, dtype=np.float32)
    assert len(th) == k
    cap = int(ns.sum()) // 2 + 16 * k + 16
    out = np.zeros(cap, dtype=simlib.REC_DTYPE)
    first = np.full(k + 1, -9, dtype=np.int32)
    kept = np.full(k, -9, dtype=np.int32)
    ovf = np.full(k, -9, dtype=np.int32)
    host = np.full(max(host_cap, 1) * 32, 0xEE, dtype=np.uint8)
    rc = _lib().batch_run(c.c_int(mode), c.c_int(sps), c.c_int(k), ptrs, ns.ctypes.data_as(c.c_void_p),
                          offs.ctypes.data_as(c.c_void_p), th.ctypes.data_as(c.c_void_p), c.c_float(scale), c.c_int(rec_cap),
                          c.c_int(1 if long_aware else 0), out.ctypes.data_as(c.c_void_p), c.c_int(cap),
                          first.ctypes.data_as(c.c_void_p), kept.ctypes.data_as(c.c_void_p), ovf.ctypes.data_as(c.c_void_p),
                          host.ctypes.data_as(c.c_void_p), c.c_int(host_cap))
    assert rc >= 0, rc
    assert first[0] == 0 and first[-1] == rc and np.all(np.diff(first) >= 0), first
    # the head of the dense list that goes straight to the host, and nothing behind it
    nh = min(rc, host_cap)
    assert host[:nh * 32].tobytes() == out[:nh].tobytes()
    assert np.all(host[nh * 32:] == 0xEE)
    for i in range(k):
        assert first[i + 1] - first[i] == max(int(kept[i]), 0)
    return [out[first[i]:first[i + 1]].copy() for i in range(k)], first, kept, ovf


def rate_goldens(sps, limit=1 << 17):
    names = helpers.golden_names() + helpers.pathological_names() + helpers.path_golden_names()
    gs = [helpers.Golden(n) for n in names]
    return [g for g in gs if g.sps == sps and len(g.x) <= limit]


# ---- 1. the reference's single-call vectors, every golden of a rate as ONE batch ----------------------------------------
@pytest.mark.parametrize("sps", [2, 4, 8, 20])
def test_goldens_of_a_rate_as_one_batch(sps):
    gs = rate_goldens(sps)
    assert len(gs) >= 3
    if sps == 2:
        assert len(gs) == 22
        lens = sorted(len(g.x) for g in gs)
        assert lens[0] == 1 and lens[-1] == 131072
        thr = {np.float32(g.thr) for g in gs}
        assert {np.float32(0.01), np.float32(0.001), np.float32(0.0), np.float32(-1.0)} <= thr
    arrays = [aligned(np.asarray(g.x, dtype=np.float32)) for g in gs]
    thrs = [g.thr for g in gs]
    offs = [1000 * i for i in range(len(gs))]
    # with lists that hold anything ...
    big = max(len(a) for a in arrays) // 8 + 64
    recs, first, kept, ovf = batch_run(1, sps, arrays, thrs, rec_cap=big, abs_offsets=offs)
    assert np.all(kept >= 0) and not ovf.any()
    for i, g in enumerate(gs):
        r = recs[i].copy()
        r["offset"] -= offs[i]
        helpers.assert_recs_match_golden(r, g)
    # ... and with the product's capacity: the preamble train of Qpaths_4msps overflows its lists and is handed back (the
    # library's host runs it through the ordinary pass); every other vector is inside its lists and equals the reference
    recs, first, kept, ovf = batch_run(1, sps, arrays, thrs)
    for i, g in enumerate(gs):
        if g.name == "Qpaths_4msps":
            assert kept[i] == -1 and ovf[i] == 1 and len(recs[i]) == 0
        else:
            assert kept[i] >= 0 and ovf[i] == 0, g.name
            helpers.assert_recs_match_golden(recs[i], g)
    if sps == 4:
        assert "Qpaths_4msps" in [g.name for g in gs]


# ---- 2. the other four formats against the ordinary pass, item by item ---------------------------------------------------
def _items_of(mode, sps):
    """a handful of items of unequal lengths per format: (data in the format's layout, threshold).  The 2 Msps vectors'
    samples, each repeated sps/2 times, are the same bursts at sps Msps."""
    out = []
    rep = sps // 2
    if mode in (0, 2):
        from gr_adsb_amd import modulator as M
        names = [n for n in helpers.golden_names() if n.startswith("g2msps")]
        for k, n in enumerate((12000, 16666, 4096, 1025, 9000)):
            z = np.load(os.path.join(helpers.GOLDEN_DIR, names[k % len(names)] + ".npz"))
            pairs = z["iq16"].reshape(-1, 2)[3000 * k:3000 * k + n]
            cut = np.repeat(pairs, rep, axis=0).reshape(-1)
            out.append((aligned(cut) if mode == 2 else aligned(M.dequantize_iq16(cut)), float(z["threshold"])))
    else:
        for k, n in enumerate((16384, 5000, 1024, 30000)):
            out.append((aligned(helpers.rise_storm_iq8(n, seed=k, offset_binary=(mode == 4), half=rep)), 0.01))
    return out


@pytest.mark.parametrize("fs", [2e6, 8e6, 12e6])
@pytest.mark.parametrize("mode", [0, 2, 3, 4])
def test_formats_equal_the_ordinary_pass(mode, fs):
    sps = int(fs // 1e6)
    items = _items_of(mode, sps)
    scale = {0: 1.0, 2: 2.0 / 32767.0, 3: 1.0 / 128.0, 4: 1.0 / 255.0}[mode]
    big = max(len(a) for a, _ in items) // 8 + 64
    recs, first, kept, ovf = batch_run(mode, sps, [a for a, _ in items], [t for _, t in items], scale=scale, rec_cap=big)
    assert np.all(kept >= 0)
    total = 0
    for i, (a, thr) in enumerate(items):
        want, _ = simlib.sim_canonical(mode, a, fs, thr, scale=scale)
        assert recs[i].tobytes() == want.tobytes(), "item %d" % i
        total += int((want["flags"] & 1).sum())
    assert total > 10                               # PDUs, not only tags


def test_batch_ignores_a_power_of_two_scale():
    """The ordinary pass runs the dot-product instances (MODE 5 / 6) for a power-of-two scale; the batch runs the generic
    conversion whatever the scale: the records must not differ."""
    for mode, scale in ((3, 2.0 ** -7), (4, 2.0 ** -6)):
        a = aligned(helpers.rise_storm_iq8(20000, seed=5, offset_binary=(mode == 4)))
        thr = 0.01 if mode == 3 else 0.04
        recs, _, kept, _ = batch_run(mode, 2, [a], [thr], scale=scale, rec_cap=4096)
        want, _ = simlib.sim_canonical(mode, a, 2e6, thr, scale=scale)
        assert kept[0] == len(want) > 0 and recs[0].tobytes() == want.tobytes()


# ---- 3. neighbours in memory ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0])
def test_items_cut_back_to_back_out_of_one_buffer(mode):
    """Items that lie back to back in ONE buffer: a burst whose bits run past the end of item k (so that its last samples
    are item k+1's first ones) and an item that starts a few samples in front of a preamble.  Each item must come out as if
    it were alone: zeros before its first and after its last sample -- for the window, the noise median and the bit slices."""
    g = helpers.Golden("g2msps_df17")
    sps, thr = g.sps, g.thr
    src = np.asarray(g.x if mode == 1 else g.iq)
    pdus = g.get("single", "pdu_offsets")
    p1, p2, p3 = int(pdus[3]), int(pdus[9]), int(pdus[15])
    al = 4 if mode == 1 else 2                    # samples per 16 bytes
    cut1 = (p1 + 8 * sps + 61 * sps) // al * al    # in the middle of the first burst's data bits
    cut2 = (p2 - 3) // al * al                      # a few samples in front of a preamble's first pulse
    cut3 = (p3 + 2 * sps) // al * al                # between a preamble's pulses: high samples right at the start
    cuts = [0, cut1, cut2, cut3, cut3 + 4096, len(src)]
    assert cuts == sorted(cuts)
    buf = aligned(src)
    items = [buf[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert float(np.max(np.abs(items[1][:16]))) ** (1 if mode == 1 else 2) >= thr          # high samples at the head of item 1
    offs = cuts[:-1]
    recs, first, kept, ovf = batch_run(mode, sps, items, [thr] * len(items), abs_offsets=offs)
    assert np.all(kept >= 0)
    n_cut = 0
    for i, it in enumerate(items):
        want, _ = simlib.sim_canonical(mode, it.copy(), g.fs, thr, abs_offset=offs[i])
        assert recs[i].tobytes() == want.tobytes(), "item %d" % i
        n_cut += len(want)
    # the seams did cost something (else the cuts were not where the bursts are): fewer PDUs than the uncut stream
    whole, _ = simlib.sim_canonical(mode, src, g.fs, thr)
    cat = np.concatenate(recs)
    assert (cat["flags"] & 1).sum() < (whole["flags"] & 1).sum()
    assert not np.array_equal(cat["offset"], whole["offset"]) or cat.tobytes() != whole.tobytes()


# ---- 4. the pack step ---------------------------------------------------------------------------------------------------------
def _small_items():
    from gr_adsb_amd import modulator as M
    out = []
    for k, n in enumerate((6000, 2500, 9000)):
        out.append(aligned(M.synth_iq(n, 2e6, 4000, seed=20 + k)))
    return out


def test_pack_with_empty_items_everywhere():
    its = _small_items()
    e = np.zeros(0, dtype=np.complex64)
    arrays = [e, its[0], e, e, its[1], its[2], e]
    recs, first, kept, ovf = batch_run(0, 2, arrays, [0.01] * len(arrays))
    assert list(kept[[0, 2, 3, 6]]) == [0, 0, 0, 0]
    assert first[0] == first[1] == 0 and first[2] == first[3] == first[4] and first[-1] == first[-2]
    for i, a in enumerate(arrays):
        if len(a):
            want, _ = simlib.sim_canonical(0, a, 2e6, 0.01)
            assert len(want) > 0 and recs[i].tobytes() == want.tobytes()
        else:
            assert len(recs[i]) == 0
    assert first[-1] == sum(len(r) for r in recs)


def test_pack_of_only_empty_items():
    e = np.zeros(0, dtype=np.float32)
    recs, first, kept, ovf = batch_run(1, 2, [e, e, e], [0.01, 0.0, -1.0])
    assert list(first) == [0, 0, 0, 0] and list(kept) == [0, 0, 0]


def test_an_overflowing_item_is_flagged_and_disturbs_nobody():
    its = _small_items()
    train = aligned(helpers.preamble_train_iq(1 << 15))
    want_train, so = simlib.sim_canonical(0, train, 2e6, 0.01)
    rec_cap = 64
    assert so.n_rec > 4 * rec_cap                   # more centres than four lists of this capacity hold
    arrays = [its[0], train, its[1], its[2]]
    recs, first, kept, ovf = batch_run(0, 2, arrays, [0.01] * 4, rec_cap=rec_cap)
    assert list(ovf) == [0, 1, 0, 0] and kept[1] == -1 and len(recs[1]) == 0
    for i in (0, 2, 3):
        want, _ = simlib.sim_canonical(0, arrays[i], 2e6, 0.01)
        assert len(want) > 0 and recs[i].tobytes() == want.tobytes()
    # with the product's capacity the same train fits (a centre every 64 samples against chunk/256 + 64 slots does not: the
    # GPU suite builds its overflow item for that formula)
    recs, first, kept, ovf = batch_run(0, 2, arrays, [0.01] * 4, rec_cap=(1 << 15) // 8)
    assert kept[1] == len(want_train) and recs[1].tobytes() == want_train.tobytes()


def test_long_aware_gate_in_a_batch():
    g = helpers.Golden("g2msps_mixed_lowsnr")
    a = aligned(np.asarray(g.x[:60000], dtype=np.float32))
    b = aligned(np.asarray(g.x[60000:100000], dtype=np.float32))
    recs, _, kept, _ = batch_run(1, 2, [a, b], [g.thr, g.thr], long_aware=True)
    with simlib.long_aware_gate():
        for i, it in enumerate((a, b)):
            want, _ = simlib.sim_canonical(1, it, g.fs, g.thr)
            assert len(want) > 0 and recs[i].tobytes() == want.tobytes()


def test_an_item_over_the_limit_is_left_to_the_host():
    lim = _lib().batch_item_max()
    assert lim == _native.BATCH_ITEM_MAX == 1 << 22
    big = aligned(np.zeros(lim + 4096, dtype=np.int8).repeat(2))          # int8 IQ: 2 bytes per sample
    small = aligned(helpers.rise_storm_iq8(4096, seed=1))
    recs, first, kept, ovf = batch_run(3, 2, [small, big, small], [0.01] * 3, scale=1.0 / 128.0, rec_cap=1024)
    assert kept[1] == -1 and kept[0] == kept[2] > 0 and recs[0].tobytes() == recs[2].tobytes()


# ---- 5. build facts ---------------------------------------------------------------------------------------------------------
def _resources():
    from gr_adsb_amd import build as B
    if not os.path.exists(B.RES):
        pytest.skip("kernel_resources.json is written by the library build")
    with open(B.RES) as f:
        return json.load(f)


def test_batch_kernels_have_no_scratch_and_no_spilled_vector_registers():
    res = _resources()
    kb = {k: v for k, v in res.items() if "k_batch" in k}
    packs = [k for k in kb if "k_batch_pack" in k]
    main = [k for k in kb if k not in packs]
    assert len(packs) == 1 and len(main) == 10, sorted(kb)       # five formats x (2 Msps, run-time tap stride)
    for k, v in kb.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
    # the names must not move the counts tests/test_abi.py holds
    assert not any("k_detect" in k or "k_order" in k or "k_resolve" in k or "k_count" in k or "k_compact" in k for k in kb)
    # what DESIGN.md records (measured facts of the build): LDS and VGPRs per workgroup, workgroups per CU
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    lds = sorted({v["lds_bytes_per_block"] for k, v in kb.items() if k in main})
    vg = [v["vgprs"] for k, v in kb.items() if k in main]
    for b in lds:
        assert ("%d" % b) in design, b
        assert (160 * 1024) // b >= 4                            # at least four workgroups (16 wavefronts) per CU by LDS
    assert max(vg) <= 128                                        # ... and by registers (512 / 4 wavefronts per SIMD)
    assert ("%d" % min(vg)) in design and ("%d" % max(vg)) in design


# ---- 6. ABI -----------------------------------------------------------------------------------------------------------------
def test_batch_item_layout_and_abi_version():
    dt = _native.BATCH_ITEM_DTYPE
    assert dt.itemsize == 32
    assert [dt.fields[n][1] for n in ("data", "n", "abs_offset", "threshold", "reserved")] == [0, 8, 16, 24, 28]
    assert _native.ABI_VERSION == 5
    assert "adsb_process_batch_device" in _native.EXPORTS and "adsb_process_batch" in _native.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    m = re.search(r"typedef struct adsb_batch_item \{(.*?)\} adsb_batch_item;", hdr, re.S)
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+);", m.group(1), re.M)
    assert [(t, n) for t, n in fields] == [("void", "data"), ("int64_t", "n"), ("int64_t", "abs_offset"), ("float", "threshold"),
                                           ("uint32_t", "reserved")]
    assert re.search(r"#define ADSB_ABI_VERSION 5\b", hdr)
    assert re.search(r"#define ADSB_BATCH_ITEM_MAX \(1ll << 22\)", hdr)
    for name in ("adsb_process_batch_device", "adsb_process_batch"):
        assert re.search(r"^int %s\(" % name, hdr, re.M)
    from gr_adsb_amd import build as B
    if os.path.exists(B.LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], stdout=subprocess.PIPE, text=True).stdout
        assert " adsb_process_batch_device" in out and " adsb_process_batch\n" in out
