"""Opt-in Conservative error correction (ADSB_FLAG_FEC_CONSERVATIVE; the decoder's error_corr="Conservative",
decoder.py:738-780), without a GPU: the host statement of the rule (adsb_mode_s_fec) against the unmodified reference
decoder's answers (tests/golden/g_fec.npz, tools/make_golden_fec.py) and against a NumPy restatement, the device kernels
k_fec / k_fec_slices on the SIMT emulator against the helper, the demod block's error_corr option, the kernels' resources,
and -- with the reference present -- the decoder downstream of repaired PDUs.  The GPU half is tests/test_gpu_fec.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g_fec.npz")
PI = (11, 17, 18, 19)
LONG_DFS = (16, 17, 18, 19, 20, 21, 24)
KNOWN_DFS = (0, 4, 5, 11) + LONG_DFS
PARITY_BITS = 0x1FE0                  # BURST_PARITY_OK | _LONG | _KNOWN_DF | DF field
FEC_BITS = N.BURST_FEC_FIXED | N.BURST_FEC_DF
W5 = np.array([16, 8, 4, 2, 1])


@pytest.fixture(scope="module")
def native():
    from gr_adsb_amd import build as b
    b.build()
    return N


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def parity_flags(b14):
    """The pre-filter bits the device gives a demodulated record (adsb_device.h: parity_flags_of)."""
    syn, df, nb = N.mode_s_syndrome(b14)
    f = df << N.BURST_DF_SHIFT
    f |= N.BURST_LONG if nb == 112 else 0
    f |= N.BURST_KNOWN_DF if nb else 0
    f |= N.BURST_PARITY_OK if df in PI and syn == 0 else 0
    return f


# ---- NumPy restatement: the decoder's table keyed by its 25-bit key, message mod x*G -----------------------------------
G = 0x1FFF409


def _pmod(v, m):
    dm = m.bit_length()
    while v.bit_length() >= dm:
        v ^= m << (v.bit_length() - dm)
    return v


def _int(bits):
    return int("".join(str(int(b)) for b in bits), 2)


def _table(L):
    t = {}
    for n in (1, 2):
        for i in range(L - n + 1):
            e = np.zeros(L, np.uint8)
            e[i:i + n] = 1
            k = _pmod(_int(e), G << 1)
            assert k not in t
            t[k] = (i, n)
    return t


TABLES = {}


def fec_numpy(b14):
    """(flags, bits14 out, first_bit, nflip) by the rule restated: the received DF's length, the 25-bit key looked up."""
    if not TABLES:
        TABLES.update({56: _table(56), 112: _table(112)})
    bits = np.unpackbits(np.asarray(b14, np.uint8))[:112]
    df = int(bits[:5] @ W5)
    flags = parity_flags(b14)
    if df not in PI or flags & N.BURST_PARITY_OK:
        return flags, np.asarray(b14, np.uint8).copy(), -1, 0
    L = 56 if df == 11 else 112
    hit = TABLES[L].get(_pmod(_int(bits[:L]), G << 1))
    if hit is None:
        return flags, np.asarray(b14, np.uint8).copy(), -1, 0
    i, n = hit
    rep = bits.copy()
    rep[i:i + n] ^= 1
    df2 = int(rep[:5] @ W5)
    if df2 in PI and (df2 == 11) == (df == 11):
        out = np.packbits(rep)
        return parity_flags(out) | N.BURST_FEC_FIXED, out, i, n
    return flags | N.BURST_FEC_DF, np.asarray(b14, np.uint8).copy(), i, n


# ---- the helper against the reference decoder ---------------------------------------------------------------------------
def test_helper_equals_the_reference_decoder(native, golden):
    """Every g_fec row: a repair the helper applies is the reference's repair (bits, DF, parity passed); a DF-changing
    repair is one the reference makes; the address/parity formats (repaired by the reference only through its aircraft
    table's absence) and unknown DFs are left as they are; under "Extended Squitter Only" the DF 17/18/19 answers agree."""
    bits = golden["bits"]
    seen = {"fixed": 0, "df": 0, "none": 0, "ap_touched_by_ref": 0, "quirk": 0}
    for i, b in enumerate(bits):
        fl, out, first, nflip = native.mode_s_fec(b)
        df0 = int(golden["df0_all"][i])
        ref_bits = golden["bits_all"][i]
        ref_repaired = not np.array_equal(ref_bits, b)
        assert fl & ~FEC_BITS == parity_flags(out), i
        if df0 in PI:
            if fl & N.BURST_FEC_FIXED:
                seen["fixed"] += 1
                assert np.array_equal(out, ref_bits) and golden["passed_all"][i] == 1, i
                assert (fl >> N.BURST_DF_SHIFT) & 31 == golden["df1_all"][i] and fl & N.BURST_PARITY_OK, i
                flipped = np.flatnonzero(np.unpackbits(out ^ b))
                assert flipped.tolist() == list(range(first, first + nflip)), i
            elif fl & N.BURST_FEC_DF:
                seen["df"] += 1
                assert ref_repaired and golden["passed_all"][i] == 1 and np.array_equal(out, b), i
                d1 = int(golden["df1_all"][i])
                assert d1 not in PI or (d1 == 11) != (df0 == 11), i
                assert np.flatnonzero(np.unpackbits(ref_bits ^ b)).tolist() == list(range(first, first + nflip)), i
            else:
                seen["none"] += 1
                assert not ref_repaired and np.array_equal(out, b) and first == -1 and nflip == 0, i
                assert bool(fl & N.BURST_PARITY_OK) == bool(golden["passed_all"][i]), i
                # the reference quirk: a reply whose last bit is 1 is never repaired (key = syndrome and last bit)
                L = int(golden["plen_all"][i])
                if not fl & N.BURST_PARITY_OK and np.unpackbits(b)[L - 1] == 1:
                    seen["quirk"] += 1
            if df0 != 11:
                assert np.array_equal(golden["bits_es"][i], ref_bits) and golden["passed_es"][i] == golden["passed_all"][i], i
        else:
            assert fl & FEC_BITS == 0 and np.array_equal(out, b) and first == -1, i
            if ref_repaired:
                seen["ap_touched_by_ref"] += 1
                assert df0 in KNOWN_DFS                   # address/parity formats only; unknown DFs have no length
        if df0 not in KNOWN_DFS:
            assert golden["plen_all"][i] == -1 and not ref_repaired, i
    assert seen["fixed"] > 700 and seen["df"] > 20 and seen["none"] > 300 and seen["quirk"] > 100, seen
    assert seen["ap_touched_by_ref"] > 0, seen


def test_numpy_restatement_agrees_with_the_helper(native, golden):
    for i, b in enumerate(golden["bits"]):
        fl, out, first, nflip = native.mode_s_fec(b)
        fl2, out2, first2, nflip2 = fec_numpy(b)
        assert (fl, first, nflip) == (fl2, first2, nflip2), i
        assert np.array_equal(out, out2), i


def test_helper_in_place_and_null_outputs(native, golden):
    lib = native.load()
    for i in range(0, len(golden["bits"]), 7):
        b = np.ascontiguousarray(golden["bits"][i]).copy()
        fl, out, _, _ = native.mode_s_fec(b)
        assert lib.adsb_mode_s_fec(b.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), None, None) == fl
        assert np.array_equal(b, out)
        # a second call, on the repaired bits, finds nothing left to repair
        want = parity_flags(out) if fl & N.BURST_FEC_FIXED else fl
        assert lib.adsb_mode_s_fec(b.ctypes.data_as(ctypes.c_void_p), None, None, None) == want


# ---- k_fec / k_fec_slices on the SIMT emulator -----------------------------------------------------------------------------
SIM_DIR = os.path.join(HERE, "sim")
FEC_SO = os.path.join(SIM_DIR, "libadsb_fec_sim.so")


@pytest.fixture(scope="module")
def fec_sim():
    srcs = [os.path.join(SIM_DIR, "fec_driver.cpp"), os.path.join(SIM_DIR, "hipsim.h"),
            os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not os.path.exists(FEC_SO) or any(os.path.getmtime(s) > os.path.getmtime(FEC_SO) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", FEC_SO])
    return ctypes.CDLL(FEC_SO)


def _records(golden):
    """The golden rows as burst records: demodulated ones with the pre-filter bits the tail gives them and assorted
    other flags; every 5th without BURST_DEMOD (bits present, no verdict)."""
    rng = np.random.default_rng(5)
    bits = golden["bits"]
    r = np.zeros(len(bits), dtype=N.BURST_DTYPE)
    r["offset"] = np.arange(len(bits)) * 1000 + 17
    r["peak"] = rng.random(len(bits), dtype=np.float32)
    r["median"] = rng.random(len(bits), dtype=np.float32)
    r["bits"] = bits
    extra = rng.choice([0, N.BURST_KEPT, N.BURST_KEPT | N.BURST_LONG_HINT, N.BURST_KEPT | N.BURST_HEAD], len(bits))
    for i in range(len(bits)):
        dem = i % 5 != 4
        r["flags"][i] = int(extra[i]) | ((N.BURST_DEMOD | parity_flags(bits[i])) if dem else 0)
    return r


def expected_fec(recs):
    """What the device must make of records: mode_s_fec on every demodulated one, every other field untouched."""
    out = recs.copy()
    for i in range(len(recs)):
        fl = int(recs["flags"][i])
        if fl & N.BURST_DEMOD:
            v, b, _, _ = N.mode_s_fec(recs["bits"][i])
            out["bits"][i] = b
            out["flags"][i] = (fl & ~PARITY_BITS) | v
    return out


def test_k_fec_on_the_emulator_equals_the_helper(native, golden, fec_sim):
    recs = _records(golden)
    want = expected_fec(recs)
    assert int(np.count_nonzero(want["flags"] & N.BURST_FEC_FIXED)) > 500
    assert int(np.count_nonzero(want["flags"] & N.BURST_FEC_DF)) > 10
    got = recs.copy()
    mirror = recs[:1000].copy()
    fec_sim.sim_fec(got.ctypes.data_as(ctypes.c_void_p), len(got), 3, mirror.ctypes.data_as(ctypes.c_void_p), len(mirror))
    assert got.tobytes() == want.tobytes()
    assert mirror.tobytes() == want[:1000].tobytes()


def test_k_fec_slices_on_the_emulator_equals_the_helper(native, golden, fec_sim):
    bits = np.ascontiguousarray(golden["bits"]).copy()
    ok = np.array([0 if i % 9 == 8 else 1 | (parity_flags(b) & 0xE0) for i, b in enumerate(bits)], dtype=np.uint8)
    want_bits, want_ok = bits.copy(), ok.copy()
    for i in range(len(bits)):
        if ok[i]:
            v, b, _, _ = N.mode_s_fec(bits[i])
            want_bits[i] = b
            want_ok[i] = 1 | (v & 0xE0) | ((v & FEC_BITS) >> 13)
    assert np.array_equal(N.demod_flags(want_ok) & (N.BURST_PARITY_OK | FEC_BITS),
                          np.array([(N.mode_s_fec(b)[0] if o else 0) & (N.BURST_PARITY_OK | FEC_BITS) for b, o in zip(bits, ok)]))
    fec_sim.sim_fec_slices(bits.ctypes.data_as(ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p), len(bits), 2)
    assert np.array_equal(bits, want_bits) and np.array_equal(ok, want_ok)


def test_k_fec_resources_fit_beside_every_k_detect():
    """k_fec runs behind a pass's compaction, i.e. beside the next pass's k_detect like the tail kernels: no scratch, no
    LDS beyond what k_detect leaves, and room for a workgroup's four wavefronts (tests/test_abi.py holds the tail's)."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    LDS_CU, VGPR_SIMD, SIMDS, GRAN = 160 * 1024, 512, 4, 1280
    alloc = lambda v: -(-v // 8) * 8                                    # noqa: E731
    gran = lambda b: -(-b // GRAN) * GRAN                               # noqa: E731
    fec = {k: v for k, v in res.items() if "k_fec" in k}
    assert len(fec) == 2                                                 # k_fec, k_fec_slices
    detect = {k: v for k, v in res.items() if "k_detect" in k}
    assert len(detect) == 35
    for name, d in detect.items():
        mode = int(re.search(r"k_detectILi(\d)E", name).group(1))
        wpb = 1 if mode in (3, 4, 5, 6) else 4
        wg_cu = min(LDS_CU // gran(d["lds_bytes_per_block"]), SIMDS * (VGPR_SIMD // alloc(d["vgprs"])) // wpb, 32)
        free_lds = LDS_CU - wg_cu * gran(d["lds_bytes_per_block"])
        per_simd = [6, 5, 5, 5] if wpb == 1 else [5, 5, 5, 5]
        for fname, f in fec.items():
            assert f["scratch_bytes_per_lane"] == 0 and f["vgpr_spills"] == 0, fname
            assert gran(f["lds_bytes_per_block"]) <= free_lds, (fname, name)
            slots = sum((VGPR_SIMD - w * alloc(d["vgprs"])) // alloc(f["vgprs"]) for w in per_simd)
            assert slots >= 4, (fname, f["vgprs"], name, d["vgprs"])


# ---- the demod block's option -------------------------------------------------------------------------------------------
class _NoGpuContext:
    """Stands in for _native.Context so that the block constructors run without a GPU."""
    made = []

    def __init__(self, fs, threshold, device=0, flags=0):
        self.args = (fs, threshold, device, flags)
        self.closed = False
        _NoGpuContext.made.append(self)

    def close(self):
        self.closed = True


@pytest.fixture
def blocks(monkeypatch):
    from gr_adsb_amd import blocks as B
    monkeypatch.setattr(N, "Context", _NoGpuContext)
    _NoGpuContext.made = []
    return B


def test_demod_error_corr_values(blocks):
    for v in ("None", "Brute Force"):
        d = blocks.demod(2e6, error_corr=v)
        assert d.error_corr == v and d._ctx.args[3] & N.FLAG_FEC_CONSERVATIVE == 0 and d.corrected == 0
    d = blocks.demod(2e6, error_corr="Conservative")
    assert d._ctx.args[3] & N.FLAG_FEC_CONSERVATIVE and d.corrected == 0
    assert blocks.demod(2e6)._ctx.args[3] == 0
    for bad in ("conservative", "", None, "Full"):
        with pytest.raises(ValueError):
            blocks.demod(2e6, error_corr=bad)


def test_pairing_a_conservative_demod_enables_fec_on_the_framers_pass(blocks):
    f = blocks.framer(2e6, 0.01, device=0)
    first = f._ctx
    assert first.args[3] == N.FLAG_FRAMER_SLICES
    blocks.demod(2e6, framer=f, error_corr="Conservative")
    assert first.closed and f._ctx is not first
    assert f._ctx.args == (2e6, 0.01, 0, N.FLAG_FRAMER_SLICES | N.FLAG_FEC_CONSERVATIVE)
    g = blocks.framer(2e6, 0.01)
    blocks.demod(2e6, framer=g, error_corr="Brute Force")
    assert g._ctx.args[3] == N.FLAG_FRAMER_SLICES
    h = blocks.framer(4e6, 0.02)
    h._nwritten = 5                                                  # (grshim's counter: the framer has run)
    with pytest.raises(RuntimeError):
        blocks.demod(4e6, framer=h, error_corr="Conservative")


def test_parity_filter_keeps_what_a_conservative_decoder_can_accept(blocks):
    P, K, D = N.BURST_PARITY_OK, N.BURST_KNOWN_DF, N.BURST_DEMOD
    f = blocks._prefilter_pass
    for fec in (False, True):
        assert f(D | K | P, 17, fec) and f(D | K | P | N.BURST_FEC_FIXED, 18, fec)
        assert not f(D | K, 17, fec) and not f(D, 3, fec)
        assert f(D | K, 20, fec) and f(D | K, 0, fec)                  # address/parity formats go through
        assert f(D | K | N.BURST_FEC_DF, 17, fec) == fec               # the decoder repairs those itself
    assert blocks.demod.__init__.__defaults__[-1] == "None"


# ---- downstream witness: the unmodified reference decoder ----------------------------------------------------------------
REF = "/root/reference/python/adsb/decoder.py"


def _stream(rng, n):
    """A message stream of a few aircraft with 1-2-bit errors on most messages (clean ones interleaved)."""
    from gr_adsb_amd import modulator as M
    icaos = [int(x) for x in rng.integers(1, 1 << 24, 6)]
    out = []
    for _ in range(n):
        df = int(rng.choice([11, 17, 17, 18, 19]))
        f = M.make_frame(df, rng, icao=int(rng.choice(icaos)))
        if df == 19:
            f[88:] = [(M.crc24(f[:88]) >> (23 - k)) & 1 for k in range(24)]
        if df == 17:
            f[32:37] = [0, 0, 1, 0, 0]                                   # identification: a callsign the table keeps
            f[88:] = [(M.crc24(f[:88]) >> (23 - k)) & 1 for k in range(24)]
        b = np.zeros(112, np.uint8)
        b[:len(f)] = f
        k = int(rng.integers(0, 4))
        if k:
            i = int(rng.integers(0, len(f) - 1))
            b[i:i + min(k, 2)] ^= 1
        out.append(b)
    # DF-changing repairs: DF 16 replies with a zero syndrome and last bit 0, received as DF 17 (bit 4)
    for _ in range(4):
        w = np.ones(112, np.uint8)
        while w[-1]:
            w[:5] = [1, 0, 0, 0, 0]
            w[5:88] = rng.integers(0, 2, 83)
            w[88:] = [(M.crc24(w[:88]) >> (23 - k)) & 1 for k in range(24)]
        w[4] ^= 1
        out.insert(int(rng.integers(0, len(out))), w)
    return out


def _decode(error_corr, stream):
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import ref_harness
    dec = ref_harness.load_reference_decoder("All Messages", error_corr, "None")
    errors = []
    for i, b in enumerate(stream):
        try:
            dec.decode_packet(({"timestamp": 1.0 + i * 1e-3, "snr": 20.0}, b.copy()))
        except Exception as e:          # random payloads reach unfinished branches of the reference decoder
            errors.append((i, type(e).__name__))
    msgs = [(port, repr(m)) for port, m, _ in dec.msgs]
    planes = {k: repr(sorted(v.items())) if isinstance(v, dict) else repr(v) for k, v in dec.plane_dict.items()}
    return msgs, planes, errors


@pytest.mark.skipif(not os.path.exists(REF), reason="needs the reference decoder")
def test_reference_decoder_downstream_of_repaired_pdus(native, monkeypatch):
    import time
    monkeypatch.setattr(time, "time", lambda: 1.7e9)
    rng = np.random.default_rng(31)
    raw = _stream(rng, 400)
    verdict = [native.mode_s_fec(np.packbits(b)) for b in raw]
    rep = [np.unpackbits(v[1])[:112] for v in verdict]
    fixed = sum(1 for v in verdict if v[0] & N.BURST_FEC_FIXED)
    dfchg = [i for i, v in enumerate(verdict) if v[0] & N.BURST_FEC_DF]
    assert fixed > 80 and len(dfchg) >= 4
    # a Conservative decoder: repaired PDUs give what raw PDUs give
    m_raw, p_raw, e_raw = _decode("Conservative", raw)
    m_rep, p_rep, e_rep = _decode("Conservative", rep)
    assert (m_rep, p_rep, e_rep) == (m_raw, p_raw, e_raw)
    assert len(p_raw) >= 3 and any(port == "decoded" for port, _ in m_raw)
    # a decoder without FEC: the same, once the PDUs only a Conservative decoder can repair are left out of both streams --
    # those whose repair changes the DF, and those received as an address/parity format, which the device leaves alone
    ap = [i for i, b in enumerate(raw) if int(b[:5] @ W5) in set(KNOWN_DFS) - set(PI)]
    assert ap
    keep = [i for i in range(len(raw)) if i not in set(dfchg) | set(ap)]
    m_c, p_c, e_c = _decode("Conservative", [raw[i] for i in keep])
    m_n, p_n, e_n = _decode("None", [rep[i] for i in keep])
    assert (m_n, p_n, e_n) == (m_c, p_c, e_c)
    # ... and without the device's repair a decoder without FEC loses messages
    m_none_raw, _, _ = _decode("None", [raw[i] for i in keep])
    assert len(m_none_raw) < len(m_n)
