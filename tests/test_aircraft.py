"""Opt-in aircraft table (ADSB_FLAG_AIRCRAFT_TABLE; the decoder's plane_dict as check_parity uses it, decoder.py:576-665),
without a GPU: the NumPy replay (tests/aircraft_replay.py) and the host statement of the rule (adsb_mode_s_aircraft) against
the unmodified reference decoder's answers (tests/golden/g_aircraft.npz, tools/make_golden_aircraft.py); the device kernels
k_air_announce / k_air_verdict / k_air_cond on the SIMT emulator against the replay, in one and in several passes against
one table; the demod block's msg_filter option; the kernels' resources.  The GPU half is tests/test_gpu_aircraft.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import aircraft_replay as A
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g_aircraft.npz")
AP_BITS = N.BURST_AP_KNOWN | N.BURST_AP_FEC


@pytest.fixture(scope="module")
def native():
    from gr_adsb_amd import build as b
    b.build()
    return N


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def sequences(golden):
    seq = golden["seq"]
    return [np.nonzero(seq == s)[0] for s in np.unique(seq)]


def parity_flags(b14):
    """The pre-filter bits the device gives a demodulated record (from adsb_mode_s_syndrome)."""
    syn, df, nb = N.mode_s_syndrome(b14)
    f = df << N.BURST_DF_SHIFT
    if nb == 112:
        f |= N.BURST_LONG
    if nb:
        f |= N.BURST_KNOWN_DF
    if df in (11, 17, 18, 19) and syn == 0:
        f |= N.BURST_PARITY_OK
    return f


# ---- the rule against the reference decoder --------------------------------------------------------------------------------
@pytest.mark.parametrize("fec", [False, True])
def test_replay_equals_the_reference_decoder(golden, fec):
    tag = "all_cons" if fec else "all_none"
    bits = golden["bits"]
    for idx in sequences(golden):
        _, added, passed = A.replay(bits[idx], fec)
        assert np.array_equal(passed, golden["passed_" + tag][idx] == 1), idx[0]
        assert np.array_equal(added, golden["added_" + tag][idx]), idx[0]


def test_golden_covers_every_case(golden):
    """The rows reach every branch of the rule: known and unknown AP replies of every AP format, repairs of AP replies
    that re-announce their AA, that announce a repaired DF 17/18/19, and that announce nothing; announcements of raw
    DF 11/17/19 replies whose repair changes the format."""
    bits = golden["bits"]
    dfs = bits[:, 0] >> 3
    known = np.zeros(len(bits), bool)
    apfec = np.zeros(len(bits), bool)
    for idx in sequences(golden):
        fl, _, _ = A.replay(bits[idx], True)
        known[idx] = (fl & N.BURST_AP_KNOWN) != 0
        apfec[idx] = (fl & N.BURST_AP_FEC) != 0
    for df in A.AP_DFS:
        assert known[dfs == df].sum() >= 10 and (~known & ~apfec)[dfs == df].sum() >= 10, df
        assert apfec[dfs == df].sum() >= 2, df
    rules = [A.rule(b, True) for b in bits]
    cond_self = sum(1 for r, f in zip(rules, apfec) if f and r[3] == r[0])
    cond_other = sum(1 for r, f in zip(rules, apfec) if f and r[3] >= 0 and r[3] != r[0])
    cond_none = sum(1 for r, f in zip(rules, apfec) if f and r[3] < 0)
    assert cond_self >= 10 and cond_other >= 10 and cond_none >= 10
    fec_df = [i for i, b in enumerate(bits) if N.mode_s_fec(b)[0] & N.BURST_FEC_DF and rules[i][1] >= 0]
    assert len(fec_df) >= 6
    # the reference raised on some rows (decoder.py:1232: self.st of TC 19 ST 0/5-7): they announce nothing
    assert golden["raised_all_none"].sum() > 0


@pytest.mark.parametrize("fec", [False, True])
def test_helper_equals_the_replay(native, golden, fec):
    for b in golden["bits"]:
        ap_fec, aa, ann, fann = N.mode_s_aircraft(b, fec)
        assert (aa, ann, ap_fec, fann) == A.rule(b, fec), b


@pytest.mark.parametrize("fec", [False, True])
def test_extended_squitter_only_needs_no_table(native, golden, fec):
    """msg_filter="Extended Squitter Only": the device's pre-filter bits alone give the decoder's verdict."""
    from gr_adsb_amd import blocks
    tag = "es_cons" if fec else "es_none"
    for b, want in zip(golden["bits"], golden["passed_" + tag]):
        fl = N.mode_s_fec(b)[0] if fec else parity_flags(b)
        pub = N.mode_s_fec(b)[1] if fec else b
        got = blocks._prefilter_pass(fl | N.BURST_DEMOD, int(pub[0]) >> 3, fec, "Extended Squitter Only")
        assert got == bool(want), b


# ---- the kernels on the SIMT emulator ----------------------------------------------------------------------------------------
SIM_DIR = os.path.join(HERE, "sim")
AIR_SO = os.path.join(SIM_DIR, "libadsb_aircraft_sim.so")


@pytest.fixture(scope="module")
def air_sim():
    srcs = [os.path.join(SIM_DIR, "aircraft_driver.cpp"), os.path.join(SIM_DIR, "hipsim.h"),
            os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not os.path.exists(AIR_SO) or any(os.path.getmtime(s) > os.path.getmtime(AIR_SO) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", AIR_SO])
    return ctypes.CDLL(AIR_SO)


class Table:
    """A device table and its step state in host memory."""

    def __init__(self, sim):
        self.keys = np.full(1 << 24, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        self.st = np.zeros(sim.sim_air_state_bytes(), dtype=np.uint8)
        self.sim = sim
        self.next = 0

    def run(self, recs, grid, fec, mirror=None):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                    # noqa: E731
        skipped = self.sim.sim_air_pass(p(recs), len(recs), grid, p(mirror) if mirror is not None else None,
                                        0 if mirror is None else len(mirror), p(self.keys), p(self.st),
                                        ctypes.c_ulonglong(self.next), int(fec))
        self.next += 1
        assert skipped == 0

    def run_slices(self, bits14, ok, grid, fec):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                    # noqa: E731
        self.sim.sim_air_slices(p(bits14), p(ok), len(ok), grid, p(self.keys), p(self.st), ctypes.c_ulonglong(self.next),
                                int(fec))
        self.next += 1


def records(bits, fec, seed=5):
    """Rows as a pass's delivered records, published as the device publishes them (after k_fec on Conservative contexts):
    every 7th without BURST_DEMOD (not published), assorted other flags."""
    rng = np.random.default_rng(seed)
    r = np.zeros(len(bits), dtype=N.BURST_DTYPE)
    r["offset"] = np.arange(len(bits)) * 1000 + 17
    r["peak"] = rng.random(len(bits), dtype=np.float32)
    r["median"] = rng.random(len(bits), dtype=np.float32)
    extra = rng.choice([0, N.BURST_KEPT, N.BURST_KEPT | N.BURST_LONG_HINT], len(bits))
    for i, b in enumerate(bits):
        if fec:
            v, rep, _, _ = N.mode_s_fec(b)
        else:
            v, rep = parity_flags(b), b
        r["bits"][i] = rep
        r["flags"][i] = int(extra[i]) | ((N.BURST_DEMOD | v) if i % 7 != 6 else 0)
    return r


def crafted(n, rng):
    """n AP replies whose (AA, last bit) is an error pattern's key -- every one a candidate of the conditional step --
    several sharing an AA, followed by replies of what they announce."""
    pats = []
    for L in (56, 112):
        for w in (1, 2):
            for i in range(L - w + 1):
                e = np.zeros(112, np.uint8)
                e[i:i + w] = 1
                pats.append((L, e))
    rows = []
    for k in range(n):
        L, e = pats[int(rng.integers(0, len(pats)))] if k % 3 else pats[k % 5]
        syn = A._mod(e, L, 24)
        dfs = (0, 4, 5) if L == 56 else (16, 20, 21, 24)
        while True:
            f = rng.integers(0, 2, 112).astype(np.uint8)
            f[:5] = [(dfs[k % len(dfs)] >> (4 - q)) & 1 for q in range(5)]
            par = A._mod(np.concatenate([f[:L - 24], np.zeros(24, np.uint8)]), L, 24) ^ syn
            f[L - 24:L] = [(par >> (23 - q)) & 1 for q in range(24)]
            if f[L - 1] == e[L - 1]:
                break
        rows.append(np.packbits(f))
    return np.array(rows, dtype=np.uint8)


@pytest.mark.parametrize("fec", [False, True])
@pytest.mark.parametrize("grid", [1, 3])
def test_kernels_equal_the_replay_in_one_pass(native, golden, air_sim, fec, grid):
    recs = records(golden["bits"], fec)
    want = A.expected_records(recs, fec, set())
    assert int(np.count_nonzero(want["flags"] & N.BURST_AP_KNOWN)) > 150
    assert (int(np.count_nonzero(want["flags"] & N.BURST_AP_FEC)) > 20) == fec
    got = recs.copy()
    mirror = recs[:500].copy()
    Table(air_sim).run(got, grid, fec, mirror)
    assert got.tobytes() == want.tobytes()
    assert mirror.tobytes() == want[:500].tobytes()


@pytest.mark.parametrize("fec", [False, True])
def test_kernels_keep_the_table_across_passes(native, golden, air_sim, fec):
    """Passes cut so that announcements and the AP replies of their addresses fall in different passes."""
    recs = records(golden["bits"], fec, seed=9)
    cuts = [0, 1, 2, 3, 50, 51, 400, 401, 402, 900, len(recs)]
    t, known = Table(air_sim), set()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = recs[lo:hi].copy()
        want = A.expected_records(recs[lo:hi], fec, known)
        t.run(got, 2, fec)
        assert got.tobytes() == want.tobytes(), (lo, hi)
    # the same sequence in one pass gives the same flags
    one = recs.copy()
    Table(air_sim).run(one, 4, fec)
    assert one.tobytes() == A.expected_records(recs, fec, set()).tobytes()


@pytest.mark.parametrize("n", [40, 1400])
def test_conditional_announcers_in_list_order(native, air_sim, n):
    """More candidates than the step's list holds (kAirCondCap = 1024) are walked by a scan of the list instead."""
    rng = np.random.default_rng(n)
    rows = crafted(n, rng)
    follow = []
    for b in rows[:200]:
        _, _, _, fann = A.rule(b, True)
        if fann >= 0:
            f = np.concatenate([[1, 0, 1, 0, 0], rng.integers(0, 2, 107)]).astype(np.uint8)        # a DF 20 reply of fann
            par = A._mod(np.concatenate([f[:88], np.zeros(24, np.uint8)]), 112, 24) ^ fann
            f[88:] = [(par >> (23 - q)) & 1 for q in range(24)]
            follow.append(np.packbits(f))
    allrows = np.concatenate([rows, np.array(follow, dtype=np.uint8).reshape(-1, 14)])
    recs = records(allrows, True, seed=n)
    want = A.expected_records(recs, True, set())
    fl = want["flags"]
    dem = (recs["flags"] & N.BURST_DEMOD) != 0
    cands = sum(1 for b in recs["bits"][dem] if A.rule(b, True)[2])        # every one a candidate of the first verdict
    assert (cands > 1024) == (n > 1024)
    assert int(np.count_nonzero(fl & N.BURST_AP_FEC)) > 30 and int(np.count_nonzero(fl & N.BURST_AP_KNOWN)) > 10
    got = recs.copy()
    Table(air_sim).run(got, 5, True)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("fec", [False, True])
def test_slices_equal_the_replay(native, golden, air_sim, fec):
    recs = records(golden["bits"], fec, seed=3)
    bits = np.ascontiguousarray(recs["bits"]).copy()
    fl = recs["flags"]
    ok = ((fl & 0xE1) | ((fl & (N.BURST_FEC_FIXED | N.BURST_FEC_DF)) >> 13)).astype(np.uint8)
    ok[(fl & N.BURST_DEMOD) == 0] = 0
    t, known = Table(air_sim), set()
    for lo, hi in ((0, 300), (300, len(ok))):
        o, b = ok[lo:hi].copy(), bits[lo:hi].copy()
        t.run_slices(b, o, 2, fec)
        want = A.expected_records(recs[lo:hi], fec, known)["flags"]
        assert np.array_equal(b, bits[lo:hi])
        assert np.array_equal(N.demod_flags(o), np.where(ok[lo:hi] != 0, want & (0xE1 | N.BURST_FEC_FIXED | N.BURST_FEC_DF | AP_BITS), 0))


def test_kernel_resources_fit_beside_every_k_detect():
    """The table step runs behind a pass's compaction, beside the next pass's k_detect, like k_fec: no scratch, no LDS
    beyond what k_detect leaves, room for a workgroup's wavefronts (tests/test_abi.py holds the tail's limits)."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    LDS_CU, VGPR_SIMD, SIMDS, GRAN = 160 * 1024, 512, 4, 1280
    alloc = lambda v: -(-v // 8) * 8                                    # noqa: E731
    gran = lambda b: -(-b // GRAN) * GRAN                               # noqa: E731
    air = {k: v for k, v in res.items() if "k_air" in k}
    assert len(air) == 3                                                 # k_air_announce, k_air_verdict, k_air_cond
    detect = {k: v for k, v in res.items() if "k_detect" in k}
    assert len(detect) == 35
    for name, d in detect.items():
        mode = int(re.search(r"k_detectILi(\d)E", name).group(1))
        wpb = 1 if mode in (3, 4, 5, 6) else 4
        wg_cu = min(LDS_CU // gran(d["lds_bytes_per_block"]), SIMDS * (VGPR_SIMD // alloc(d["vgprs"])) // wpb, 32)
        free_lds = LDS_CU - wg_cu * gran(d["lds_bytes_per_block"])
        per_simd = [6, 5, 5, 5] if wpb == 1 else [5, 5, 5, 5]
        for fname, f in air.items():
            assert f["scratch_bytes_per_lane"] == 0 and f["vgpr_spills"] == 0 and f["sgpr_spills"] == 0, fname
            assert gran(f["lds_bytes_per_block"]) <= free_lds, (fname, name)
            slots = sum((VGPR_SIMD - w * alloc(d["vgprs"])) // alloc(f["vgprs"]) for w in per_simd)
            assert slots >= 4, (fname, f["vgprs"], name, d["vgprs"])


# ---- the demod block's option --------------------------------------------------------------------------------------------
class _NoGpuContext:
    """Stands in for _native.Context so that the block constructors run without a GPU."""

    def __init__(self, fs, threshold, device=0, flags=0):
        self.args = (fs, threshold, device, flags)

    def close(self):
        pass


@pytest.fixture
def blocks(monkeypatch):
    from gr_adsb_amd import blocks as B
    monkeypatch.setattr(N, "Context", _NoGpuContext)
    return B


def test_demod_msg_filter_values(blocks):
    T = N.FLAG_AIRCRAFT_TABLE
    assert blocks.demod(2e6).msg_filter is None and blocks.demod(2e6)._ctx.args[3] == 0
    assert blocks.demod(2e6, parity_filter=True, msg_filter="All Messages")._ctx.args[3] == T
    assert blocks.demod(2e6, parity_filter=True, msg_filter="All Messages", improved=True)._ctx.args[3] == T
    assert blocks.demod(2e6, parity_filter=True, msg_filter="All Messages",
                        error_corr="Conservative")._ctx.args[3] == T | N.FLAG_FEC_CONSERVATIVE
    assert blocks.demod(2e6, msg_filter="All Messages")._ctx.args[3] == 0           # nothing filtered: no table
    assert blocks.demod(2e6, parity_filter=True, msg_filter="Extended Squitter Only")._ctx.args[3] == 0
    for bad in ("all messages", "", "None", 0):
        with pytest.raises(ValueError):
            blocks.demod(2e6, msg_filter=bad)
    f = blocks.framer(2e6, 0.01)
    with pytest.raises(ValueError):
        blocks.demod(2e6, framer=f, parity_filter=True, msg_filter="All Messages")
    blocks.demod(2e6, framer=blocks.framer(2e6, 0.01), parity_filter=True, msg_filter="Extended Squitter Only")


def test_prefilter_with_msg_filter(blocks):
    P, K, D, KN, AF = N.BURST_PARITY_OK, N.BURST_KNOWN_DF, N.BURST_DEMOD, N.BURST_AP_KNOWN, N.BURST_AP_FEC
    f = blocks._prefilter_pass
    for fec in (False, True):
        for df in A.AP_DFS:
            assert f(D | K, df, fec) and f(D | K, df, fec, None)                     # the default: they go through
            assert not f(D | K, df, fec, "All Messages")
            assert f(D | K | KN, df, fec, "All Messages")
            assert f(D | K | AF, df, fec, "All Messages") == fec
            assert not f(D | K | KN, df, fec, "Extended Squitter Only")
        assert f(D | K | P, 11, fec, "All Messages") and not f(D | K | P, 11, fec, "Extended Squitter Only")
        assert f(D | K | P, 17, fec, "Extended Squitter Only") and not f(D | K, 18, fec, "Extended Squitter Only")
        assert f(D | K | N.BURST_FEC_DF, 19, fec, "Extended Squitter Only") == fec
