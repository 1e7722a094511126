"""The soft-decision CRC repair (ADSB_FLAG_FEC_SOFT; include/adsb_hip.h: SOFT REPAIR) without a GPU: the shipped kernels of
gr_adsb_amd/csrc/adsb_softfec_device.h on the SIMT emulator (tests/sim/softfec_driver.cpp) and the host rule
adsb_mode_s_soft_fec, byte for byte against the plain restatement tests/softfec_replay.py, on the hand-built records of
tests/softfec_cases.py; the restatement itself on a synthetic low-SNR stream; the ABI, the new unit's resources and the
demod block's keyword."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import softfec_cases as C
import softfec_replay as SR
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
SOFT_SO = os.path.join(SIM_DIR, "libadsb_softfec_sim.so")
CSRC = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    srcs = [os.path.join(SIM_DIR, "softfec_driver.cpp"), os.path.join(SIM_DIR, "hipsim.h"),
            os.path.join(CSRC, "adsb_softfec_device.h"), os.path.join(CSRC, "adsb_reply_device.h")]
    if not os.path.exists(SOFT_SO) or any(os.path.getmtime(s) > os.path.getmtime(SOFT_SO) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", SOFT_SO])
    return ctypes.CDLL(SOFT_SO)


@pytest.fixture(scope="module")
def cases():
    return C.build(2)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rule_struct(rule):
    return N.SOFT_FEC_RULE(rule["n_weak"], rule["max_flips"], rule["min_key"], 0)


FILL = 0xEE


def run_records(sim, data, n, recs, rule, grid, mode=1, scale=1.0, sps=2, origin=C.ORIGIN, spare=5, mirror_cap=None):
    """k_soft_fec over recs followed by `spare` qualifying records past n_kept; -> (list, mirror, rows), each of capacity size"""
    n_kept = len(recs)
    cap = n_kept + spare
    lst = np.concatenate([recs, np.resize(recs, spare)]) if n_kept else np.zeros(spare, dtype=SR.REC_DTYPE)
    mirror_cap = n_kept // 2 if mirror_cap is None else mirror_cap
    mirror = lst[:mirror_cap].copy()
    rows = np.full(cap, FILL, dtype=np.uint8).repeat(8).view(SR.SOFT_DTYPE)
    rs = rule_struct(rule)
    rc = sim.sim_soft_records(ctypes.c_int(mode), _p(data), ctypes.c_longlong(n), ctypes.c_longlong(origin), ctypes.c_float(scale),
                              ctypes.c_int(sps), ctypes.byref(rs), _p(lst), ctypes.c_int(n_kept), ctypes.c_int(cap),
                              _p(mirror) if mirror_cap else None, ctypes.c_int(mirror_cap), _p(rows), ctypes.c_int(grid))
    assert rc == 0
    return lst, mirror, rows


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


def check_records(sim, data, n, x, recs, rule, grid, **kw):
    want, want_rows = SR.replay_records(recs, x, kw.get("origin", C.ORIGIN), kw.get("sps", 2), rule)
    lst, mirror, rows = run_records(sim, data, n, recs, rule, grid, **kw)
    k = len(recs)
    same(lst[:k], want)
    same(rows[:k], want_rows)
    same(mirror, want[:len(mirror)])
    same(lst[k:], np.resize(recs, len(lst) - k))                                        # past n_kept: untouched
    assert rows[k:].tobytes() == bytes([FILL]) * 8 * (len(rows) - k)
    return want, want_rows


# ---- the cases reach their seams: from the restatement alone -------------------------------------------------------------

def outcome(cases, rule):
    recs = cases.records()
    out, rows = SR.replay_records(recs, cases.x, C.ORIGIN, 2, C.RULES[rule])
    by = {}
    for k, name in enumerate(cases.names):
        by[name] = (SR.unpack(out["bits"][k]), int(out["flags"][k]), rows[k], recs[k])
    return by


def repaired_to(entry, truth):
    bits, flags, row, raw = entry
    return (row["nflip"] > 0 and np.array_equal(bits, truth) and flags & SR.FEC_FIXED and flags & SR.PARITY_OK
            and sorted(np.flatnonzero(bits != SR.unpack(raw["bits"]))) == [b for b in row["bit"] if b != 0xFF])


def untouched(entry, ncand=None):
    bits, flags, row, raw = entry
    return (row["nflip"] == 0 and np.array_equal(SR.pack(bits), raw["bits"]) and flags == raw["flags"]
            and (ncand is None or row["ncand"] == ncand))


def test_cases_reach_their_seams(cases):
    assert len(cases.names) <= 40 and len(cases.x) == 1 << 12
    d = outcome(cases, "default")
    # 1. zero syndrome, no DEMOD, FEC_DF set, a DF outside 11/17/18/19: untouched, zero row
    for name in ("clean", "no_demod", "fec_df", "df20"):
        assert untouched(d[name], 0) and d[name][2].tobytes() == bytes(8), name
    # 2. one wrong bit: the weakest / at rank n_weak
    assert repaired_to(d["one_weakest"], cases.truth["one_weakest"]) and list(d["one_weakest"][2]["bit"]) == [40, 255, 255, 255, 255]
    assert untouched(d["one_outside"], 8)
    # 3. three scattered wrong bits inside the 8 weakest; with max_flips = 2
    assert repaired_to(d["three_scattered"], cases.truth["three_scattered"]) and list(d["three_scattered"][2]["bit"]) == [8, 66, 91, 255, 255]
    assert untouched(outcome(cases, "two_flips")["three_scattered"], 8)
    # 4. a key tie across the n_weak boundary goes to the lower bit index
    assert d["tie_lower_wrong"][2]["nflip"] == 1 and list(d["tie_lower_wrong"][2]["bit"][:1]) == [33]
    assert untouched(d["tie_higher_wrong"], 8)
    # 5. lane and word seams; a wrong DF bit is never a candidate
    caps = outcome(cases, "caps")
    assert untouched(d["seams"], 8) and repaired_to(caps["seams"], cases.truth["seams"]) and list(caps["seams"][2]["bit"]) == [5, 63, 64, 111, 255]
    assert untouched(d["df_bit"]) and untouched(caps["df_bit"]) and SR.df_of(d["df_bit"][0]) == 19
    # 6. DF 11: bits 56.. are ignored however weak, bit 55 is repaired
    assert repaired_to(d["df11"], cases.truth["df11"]) and list(d["df11"][2]["bit"]) == [55, 255, 255, 255, 255] and d["df11"][2]["ncand"] == 8
    # 7. the weight-6 codeword: two 3-subsets match, the smaller mask wins in both rank orders
    one, two = C.weight6()
    assert (one, two) == C.find_weight6() and min(one + two) >= 5
    assert repaired_to(d["weight6_true_first"], cases.truth["weight6_true_first"]) and list(d["weight6_true_first"][2]["bit"][:3]) == one
    other = d["weight6_other_first"]
    assert other[2]["nflip"] == 3 and list(other[2]["bit"][:3]) == two and not np.array_equal(other[0], cases.truth["weight6_other_first"])
    assert sorted(np.flatnonzero(other[0] != cases.truth["weight6_other_first"])) == sorted(one + two)
    # 8. samples without a quotient, and min_key at 0, between two candidates' keys, at 1
    assert repaired_to(d["no_quotient"], cases.truth["no_quotient"]) and list(d["no_quotient"][2]["bit"][:2]) == [21, 26]
    k = SR.sample_keys(cases.x, int(d["no_quotient"][3]["offset"]) - C.ORIGIN, 2)
    assert list(k[21:27]) == [1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    one_key = outcome(cases, "min_key_one")
    assert repaired_to(one_key["no_quotient"], cases.truth["no_quotient"]) and one_key["no_quotient"][2]["ncand"] == 3
    assert untouched(one_key["three_scattered"], 0)
    assert untouched(outcome(cases, "min_key_between")["three_scattered"], 6)
    # 9. the caps: five wrong bits at ranks 11..15 of sixteen; n_weak = 1
    assert untouched(d["five_deep"], 8) and repaired_to(caps["five_deep"], cases.truth["five_deep"]) and caps["five_deep"][2]["nflip"] == 5
    w1 = outcome(cases, "one_weak")
    assert repaired_to(w1["one_weakest"], cases.truth["one_weakest"]) and untouched(w1["three_scattered"], 1)


# ---- the emulated kernels and the host rule against the restatement ------------------------------------------------------

@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("rule", sorted(C.RULES))
def test_records_kernel_equals_the_replay(sim, cases, rule, grid):
    recs = np.resize(cases.records(), 40)               # 40 records: three workgroups of four wavefronts take several rounds
    check_records(sim, cases.x, len(cases.x), cases.x, recs, C.RULES[rule], grid)


def test_records_kernel_edges(sim, cases):
    recs = cases.records()
    for n_kept, mirror_cap in ((0, 0), (1, 1), (len(recs), 0), (len(recs), len(recs))):
        check_records(sim, cases.x, len(cases.x), cases.x, recs[:n_kept], C.RULES["default"], 2, mirror_cap=mirror_cap)
    # a burst that leaves the buffer: the samples past its end read as zero (key 1, a candidate)
    r = recs[:2].copy()
    r["offset"] = [C.ORIGIN + len(cases.x) - 100, C.ORIGIN - 50]
    check_records(sim, cases.x, len(cases.x), cases.x, r, C.RULES["caps"], 1)


def test_records_kernel_at_ten_samples_per_microsecond(sim):
    B = C.build(10)
    want, rows = check_records(sim, B.x, len(B.x), B.x, B.records(), C.RULES["default"], 1, sps=10)
    assert list(rows["nflip"][:2]) == [1, 3] and not rows["nflip"][2:].any()


@pytest.mark.parametrize("rule", sorted(C.RULES))
def test_slices_kernel_equals_the_replay(sim, cases, rule):
    bits14, ok, tags = C.slices_of(np.resize(cases.records(), 40))
    want_bits, want_ok, want_rows = SR.replay_slices(bits14, ok, tags, cases.x, 2, C.RULES[rule])
    for grid in (1, 3):
        b, o = bits14.copy(), ok.copy()
        rows = np.full(len(ok), FILL, dtype=np.uint8).repeat(8).view(SR.SOFT_DTYPE)
        rs = rule_struct(C.RULES[rule])
        sim.sim_soft_slices(_p(cases.x), ctypes.c_longlong(len(cases.x)), _p(tags), ctypes.c_int(2), ctypes.byref(rs), _p(b), _p(o),
                            ctypes.c_int(len(ok)), _p(rows), ctypes.c_int(grid))
        same(b, want_bits), same(o, want_ok), same(rows, want_rows)
    if rule == "default":
        fixed = want_rows["nflip"] != 0
        assert fixed.any() and ((want_ok & 2) != 0).tolist() == fixed.tolist()                  # ok[] bit 1 reports the repair


@pytest.mark.parametrize("rule", sorted(C.RULES))
def test_host_rule_equals_the_replay(cases, rule):
    r = C.RULES[rule]
    for rec in cases.records():
        bits = SR.unpack(rec["bits"])
        key = SR.sample_keys(cases.x, int(rec["offset"]) - C.ORIGIN, 2)
        want_bits, fixed, want_row = SR.soft_rule(bits, key, **r)
        fl, out, row = N.mode_s_soft_fec(rec["bits"], key, **r)
        assert out.tobytes() == SR.pack(want_bits).tobytes() and row.tobytes() == want_row.tobytes()
        assert fl == SR.prefilter_flags(want_bits) | (SR.FEC_FIXED if fixed else 0)


def formats(rng, n):
    """(mode, raw samples, scale, float32 |IQ|^2 as the device converts them) for the five input formats"""
    from oracle import adsb_oracle as O
    iq = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(0.3)
    i16 = rng.integers(-2000, 2000, 2 * n).astype(np.int16)
    i8 = rng.integers(-128, 128, 2 * n).astype(np.int8)
    u8 = rng.integers(0, 256, 2 * n).astype(np.uint8)
    return [(0, iq, 1.0, O.mag2(iq)), (1, O.mag2(iq), 1.0, O.mag2(iq)), (2, i16, 1.0 / 32768, O.mag2_iq16(i16, 1.0 / 32768)),
            (3, i8, 1.0 / 128, O.mag2_iq8(i8, 1.0 / 128)), (4, u8, 1.0 / 255, O.mag2_iq8(u8, 1.0 / 255, offset_binary=True))]


@pytest.mark.parametrize("k", range(5))
def test_records_kernel_reads_every_input_format(sim, k):
    """Replies whose two or three weakest candidates (by the format's own converted samples) are wrong: repaired in every format"""
    rng = np.random.default_rng(40 + k)
    mode, data, scale, x = formats(rng, 1 << 12)[k]
    recs = np.zeros(12, dtype=SR.REC_DTYPE)
    for t in range(len(recs)):
        p = int(rng.integers(0, len(x) - 240))
        key = SR.sample_keys(x, p, 2)
        f = C.frame(int(rng.choice([11, 17, 18, 19])), rng)
        wrong = SR.candidates(key, SR.length_of(SR.df_of(f)), 8, 0.0)[:2 + t % 2]
        bits = C.flipped(f, wrong)
        recs[t] = (p + 77, 1.0, 0.1, SR.pack(bits), SR.DEMOD | SR.prefilter_flags(bits))
    want, rows = check_records(sim, data, len(x), x, recs, C.RULES["default"], 2, mode=mode, scale=scale, origin=77)
    assert (rows["nflip"] >= 1).all() and (want["flags"] & SR.FEC_FIXED).all()


# ---- the restatement on a synthetic low-SNR stream ---------------------------------------------------------------------------

def stream_counts(seed, n_weak, max_flips, lo_db=6, hi_db=14):
    from gr_adsb_amd import modulator as M
    from oracle import adsb_oracle as O
    fs, sps = 2e6, 2
    z, truth = M.synth_iq(1 << 20, fs, 1500, seed, noise_power=1e-3, snr_db_range=(lo_db, hi_db), return_truth=True)
    x = O.mag2(z)
    out = O.run_stream(x, fs, 0.004)
    tmap = {s: (df, b) for s, df, b in truth}
    tot = dict(frames=0, bad=0, cons=0, soft=0, wrong=0, garbage=0, garbage_soft=0)
    for off, bits in zip(out["pdu_offsets"], out["pdu_bits"]):
        off, df = int(off), SR.df_of(bits)
        if df not in SR.PI_DFS:
            continue
        L = SR.length_of(df)
        real = off in tmap and tmap[off][0] == df
        S = SR.syndrome(bits, L)
        if not real:
            tot["garbage"] += 1
            if S and SR.conservative(bits, L) is None and SR.soft_rule(bits, SR.sample_keys(x, off, sps), n_weak, max_flips)[1]:
                tot["garbage_soft"] += 1
            continue
        tb = np.array(tmap[off][1][:L], dtype=np.uint8)
        tot["frames"] += 1
        if S == 0:
            continue
        tot["bad"] += 1
        c = SR.conservative(bits, L)
        if c is not None:
            b2 = bits.copy(); b2[c] ^= 1
            tot["cons"] += 1; tot["wrong"] += int(not np.array_equal(b2[:L], tb))
            continue
        b2, fixed, _ = SR.soft_rule(bits, SR.sample_keys(x, off, sps), n_weak, max_flips)
        if fixed:
            tot["soft"] += 1; tot["wrong"] += int(not np.array_equal(b2[:L], tb))
    return tot


def test_replay_counts_on_the_synthetic_stream():
    """Seeds 0..3 of a 2^20-sample stream at 6..14 dB, DF 17: of the transmitted frames detected at their true offset the
    Conservative rule repairs 57, the soft rule at 8 / 3 another 130, every one equal to the transmitted frame, and no false
    detection is "repaired" by the soft rule (counts of ONE synthetic model, not of real traffic)."""
    tot = {}
    for seed in range(4):
        for k, v in stream_counts(seed, 8, 3).items():
            tot[k] = tot.get(k, 0) + v
    print(tot)
    assert tot["frames"] == 1318 and tot["bad"] == 419
    assert tot["cons"] == 57 and tot["soft"] == 130 and tot["wrong"] == 0
    assert tot["garbage"] == 17 and tot["garbage_soft"] == 0


# ---- ABI, arguments, resources, the block --------------------------------------------------------------------------------

def test_abi_header_and_symbols():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_ABI_VERSION 5\b", src) and N.ABI_VERSION == 5
    assert re.search(r"#define ADSB_FLAG_FEC_SOFT 16384u", src) and N.FLAG_FEC_SOFT == 16384
    for sym in ("adsb_set_soft_fec", "adsb_last_soft", "adsb_mode_s_soft_fec"):
        assert sym in N.EXPORTS and re.search(r"^\w+ %s\(" % sym, src, re.M) and hasattr(N.load(), sym)
    assert "SOFT REPAIR" in src and "typedef struct adsb_soft_fix" in src and "typedef struct adsb_soft_fec_rule" in src
    assert N.SOFT_DTYPE == SR.SOFT_DTYPE and N.SOFT_DTYPE.itemsize == 8 and ctypes.sizeof(N.SOFT_FEC_RULE) == 16
    assert [N.SOFT_DTYPE.fields[k][1] for k in N.SOFT_DTYPE.names] == [0, 1, 2, 7]
    assert N.SOFT_FEC_DEFAULTS == SR.DEFAULTS == dict(n_weak=8, max_flips=3, min_key=0.0)
    assert callable(N.Context.set_soft_fec) and callable(N.Context.last_soft)
    dev = open(os.path.join(CSRC, "adsb_device.h")).read()
    assert '#include "adsb_reply_device.h"' in dev and "includes nothing" not in dev


def test_false_repair_odds_stated_in_the_header():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    for n_weak, max_flips, text in ((8, 3, "5.5e-6"), (16, 5, "4.1e-4")):
        T = sum(math.comb(n_weak, k) for k in range(1, max_flips + 1))
        assert "T = %d" % T in src and text in src and "%.1e" % (T / 2 ** 24) == text.replace("e-", "e-0")


def test_create_refuses_the_flag_combinations():
    lib = N.load()
    h = ctypes.c_void_p()
    for bad in (N.FLAG_STREAM_DECODE, N.FLAG_FRAMER_SLICES, N.FLAG_STREAM_DECODE | N.FLAG_STREAM_DECODE_SHARED):
        assert lib.adsb_create(2e6, 0.01, 0, N.FLAG_FEC_SOFT | bad, ctypes.byref(h)) == -22 and not h.value
    # the argument checks come first: without a device the combinations that are allowed get as far as -ENODEV (or succeed)
    for good in (0, N.FLAG_FEC_CONSERVATIVE, N.FLAG_AIRCRAFT_TABLE | N.FLAG_DECODE | N.FLAG_PLANE_AGES, N.FLAG_CONFIDENCE | N.FLAG_TIMING,
                 N.FLAG_LONG_AWARE_GATE):
        rc = lib.adsb_create(2e6, 0.01, 0, N.FLAG_FEC_SOFT | good, ctypes.byref(h))
        assert rc in (0, -19), rc
        if rc == 0:
            lib.adsb_destroy(h)
            h = ctypes.c_void_p()


def test_host_rule_arguments():
    rng = np.random.default_rng(3)
    f = C.frame(17, rng)
    key = np.full(112, 0.1, dtype=np.float32)
    key[[50, 60]] = 0.9
    bad = C.flipped(f, [50, 60])
    lib = N.load()
    out, row = np.zeros(14, dtype=np.uint8), np.zeros(1, dtype=N.SOFT_DTYPE)
    # a NULL rule is the defaults; out and fix may be NULL
    fl = lib.adsb_mode_s_soft_fec(_p(SR.pack(bad)), _p(key), None, _p(out), _p(row))
    assert fl & N.BURST_FEC_FIXED and fl & N.BURST_PARITY_OK and out.tobytes() == SR.pack(f).tobytes() and list(row[0]["bit"][:2]) == [50, 60]
    assert lib.adsb_mode_s_soft_fec(_p(SR.pack(bad)), _p(key), None, None, None) == fl
    # in and out may be the same array; a clean reply and an address/parity format come back as they are, zero row
    buf = SR.pack(bad)
    lib.adsb_mode_s_soft_fec(_p(buf), _p(key), None, _p(buf), None)
    assert buf.tobytes() == SR.pack(f).tobytes()
    for same_bits in (f, np.concatenate([[1, 0, 1, 0, 0], bad[5:]]).astype(np.uint8)):
        fl, out, row = N.mode_s_soft_fec(SR.pack(same_bits), key)
        assert not fl & N.BURST_FEC_FIXED and out.tobytes() == SR.pack(same_bits).tobytes() and row.tobytes() == bytes(8)
    # NaN keys are no candidates
    key2 = key.copy(); key2[50] = np.nan
    fl, out, row = N.mode_s_soft_fec(SR.pack(bad), key2)
    assert not fl & N.BURST_FEC_FIXED and row["ncand"] == 8 and row["nflip"] == 0


def test_kernel_resources_of_the_new_unit():
    """Both kernels exist for every input format, with no scratch and no spills; the unit is in the build's lists."""
    from gr_adsb_amd import build as B
    B.build()
    assert B.SOFTFEC_SOURCE == "adsb_softfec.hip" and {"adsb_softfec.hip", "adsb_softfec.h", "adsb_softfec_device.h", "adsb_reply_device.h"} <= set(B.DEPS)
    res = json.load(open(B.RES_SOFTFEC))
    names = sorted(res)
    assert len(names) == 6 and sum("k_soft_fec_slices" in k for k in names) == 1 and all("k_soft_fec" in k for k in names)
    for k, v in res.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
        assert v["lds_bytes_per_block"] == 4 * 16 * 4, (k, v)             # 16 syndromes per wavefront
    assert not any("k_soft_fec" in k for k in json.load(open(B.RES)))     # and none of them in the main unit


class _NoGpuContext:
    """Stands in for _native.Context so that the block constructors run without a GPU."""
    made = []

    def __init__(self, fs, threshold, device=0, flags=0):
        self.args = (fs, threshold, device, flags)
        self.rule = None
        _NoGpuContext.made.append(self)

    def set_soft_fec(self, **kw):
        self.rule = kw

    def close(self):
        pass


@pytest.fixture
def blocks(monkeypatch):
    from gr_adsb_amd import blocks as B
    monkeypatch.setattr(N, "Context", _NoGpuContext)
    return B


def test_demod_soft_fec_keyword(blocks):
    d = blocks.demod(2e6)
    assert d._ctx.args[3] == 0 and d.soft_fec is None and d.soft_corrected == 0 and d._ctx.rule is None
    d = blocks.demod(2e6, soft_fec=True)
    assert d._ctx.args[3] == N.FLAG_FEC_SOFT and d.soft_fec == N.SOFT_FEC_DEFAULTS and d._ctx.rule is None and d.corrected == 0
    d = blocks.demod(2e6, soft_fec={"n_weak": 12, "max_flips": 4}, error_corr="Conservative", parity_filter=True, msg_filter="All Messages")
    assert d._ctx.args[3] == N.FLAG_FEC_SOFT | N.FLAG_FEC_CONSERVATIVE | N.FLAG_AIRCRAFT_TABLE
    assert d._ctx.rule == dict(n_weak=12, max_flips=4, min_key=0.0) == d.soft_fec
    # error_corr is untouched: "Brute Force" stays "None"
    assert blocks.demod(2e6, error_corr="Brute Force")._ctx.args[3] == 0
    for bad in (False, 1, "on", {"weak": 3}):
        with pytest.raises(ValueError):
            blocks.demod(2e6, soft_fec=bad)
    fr = blocks.framer(2e6, 0.01)
    with pytest.raises(ValueError):
        blocks.demod(2e6, framer=fr, soft_fec=True)
    assert "Brute Force" in blocks.demod.__init__.__doc__ and "soft_fec" in blocks.demod.__init__.__doc__
