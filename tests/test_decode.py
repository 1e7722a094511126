"""ADSB_FLAG_DECODE on the CPU: the decoder's message decoding (decode_message / decode_me, the CPR global decode,
update_plane, the published ports) against tests/golden/g_decode.npz -- the reference decoder's answers under both msg_filter
and error_corr values.  A plain-Python replay (tests/decode_replay.py), the host function that turns a row into the
reference's PDU (_native.decoded_pdu), the emulated kernels (tests/sim/decode_driver.cpp: the product's own sort included;
the sort alone is tests/test_decode_sort.py) and the kernels' resources."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import decode_replay as D
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
DEC_SO = os.path.join(SIM_DIR, "libadsb_decode_sim.so")
GOLD = os.path.join(HERE, "golden", "g_decode.npz")
CONFIGS = (("all_none", "All Messages", "None"), ("all_cons", "All Messages", "Conservative"),
           ("es_none", "Extended Squitter Only", "None"), ("es_cons", "Extended Squitter Only", "Conservative"))
NAN_BITS = 0x7FF8000000000000


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def seq_slices(seq):
    cut = np.flatnonzero(np.diff(seq)) + 1
    b = np.concatenate([[0], cut, [len(seq)]])
    return [slice(int(b[i]), int(b[i + 1])) for i in range(len(b) - 1)]


def expected(g, tag):
    """The golden rows of one configuration as DECODED_DTYPE (speed / heading: checked separately, as float64 bits)."""
    n = len(g["bits"])
    r = np.zeros(n, dtype=N.DECODED_DTYPE)
    r["port"] = g["port_" + tag]
    r["df"] = g["df_" + tag]
    r["icao"] = g["icao_" + tag]
    r["bits"] = g["bits"] ^ g["pfix_" + tag]
    has = g["has_" + tag] == 1
    vel = g["speed_" + tag] != NAN_BITS
    r["present"] = (has * N.DEC_HAS_PLANE) | (g["csset_" + tag] * N.DEC_HAS_CALLSIGN) | (g["altset_" + tag] * N.DEC_HAS_ALTITUDE) \
        | (vel * N.DEC_HAS_VELOCITY)
    r["callsign"] = [bytes(c) for c in g["cs_" + tag]]
    r["altitude"] = g["alt_" + tag]
    r["vertical_rate"] = g["vrate_" + tag]
    r["latitude"] = g["lat_" + tag].view(np.float64)
    r["longitude"] = g["lon_" + tag].view(np.float64)
    r["num_msgs"] = g["nmsgs_" + tag]
    return r


def check_rows(got, g, tag, idx=slice(None)):
    """Rows (DECODED_DTYPE) against the golden rows idx of configuration tag, float64 fields by their bits."""
    exp = expected(g, tag)[idx]
    assert len(got) == len(exp)
    for k in ("port", "df", "icao", "bits", "present", "callsign", "altitude", "vertical_rate", "num_msgs"):
        bad = np.flatnonzero(np.any((got[k] != exp[k]).reshape(len(got), -1), axis=1))
        assert len(bad) == 0, (tag, k, bad[:5], got[k][bad[:3]], exp[k][bad[:3]])
    for k in ("latitude", "longitude"):
        assert np.array_equal(got[k].view(np.uint64), exp[k].view(np.uint64)), (tag, k)
    vel = (got["present"] & N.DEC_HAS_VELOCITY) != 0
    assert np.array_equal(vel, g["speed_" + tag][idx] != NAN_BITS)
    sp = np.full(len(got), NAN_BITS, np.uint64)
    hd = np.full(len(got), NAN_BITS, np.uint64)
    for i in np.flatnonzero(vel):
        s, h = D.speed_heading(int(got["velocity_we"][i]), int(got["velocity_sn"][i]))
        sp[i], hd[i] = D.f64bits(s), D.f64bits(h)
    assert np.array_equal(sp, g["speed_" + tag][idx]) and np.array_equal(hd, g["heading_" + tag][idx]), tag


def replay_rows(g, filt, corr):
    import decode_streams as S
    rs = []
    for sl in seq_slices(g["seq"]):
        rs += D.Decoder(filt, corr).rows(g["bits"][sl], g["ts"][sl])
    return S.to_rows(rs)


# ---- the replay and the golden ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_replay_equals_golden(g, tag, filt, corr):
    check_rows(replay_rows(g, filt, corr), g, tag)


def test_golden_covers_every_class(g):
    bits = np.unpackbits(g["bits"], axis=1)
    fld = lambda lo, n: bits[:, lo:lo + n].dot(1 << np.arange(n - 1, -1, -1))      # noqa: E731
    df, sub, tc, st = fld(0, 5), fld(5, 3), fld(32, 5), fld(37, 3)
    port = g["port_all_cons"]
    dfs = set(df[port != 0].tolist()) | set(g["df_all_none"][g["has_all_none"] == 1].tolist())
    assert {0, 4, 5, 11, 16, 17, 18, 19, 20, 21} <= dfs
    ok = port == 1
    # callsigns: all 64 codes in published identifications
    codes = set()
    for i in np.flatnonzero(ok & (df == 17) & (tc >= 1) & (tc <= 4)):
        codes |= {int(bits[i, 40 + 6 * k:46 + 6 * k].dot(1 << np.arange(5, -1, -1))) for k in range(8)}
    assert codes == set(range(64))
    assert {1, 2, 3, 4} <= set(tc[ok].tolist())
    # every raising class, and ST 3/4, TC 0 / 5-8 / 20-31
    raised = g["port_all_none"] == 3
    assert (raised & (df == 18) & np.isin(sub, (2, 3, 5))).sum() >= 3
    assert set(st[raised & (tc == 19)].tolist()) >= {0, 5, 6, 7}
    assert (g["port_all_none"] == 2).sum() >= 20
    # positions: fixes in every NL zone of both hemispheres, longitudes of both signs, NaN fixes that set the altitude
    lat = g["lat_all_none"].view(np.float64)
    lon = g["lon_all_none"].view(np.float64)
    fix = ~np.isnan(lat)
    zones = {(D.nl(x), x > 0) for x in lat[fix]}
    assert {(z, h) for z in range(1, 60) for h in (True, False)} <= zones
    assert (lon[fix] < 0).any() and (lon[fix] > 0).any()
    pos = (df == 17) & (tc >= 9) & (tc <= 18)
    assert (pos & (g["altset_all_none"] == 1) & ~fix).sum() > 10
    assert (pos & (g["port_all_none"] == 0)).sum() > 50 and (pos & (g["port_all_none"] == 1)).sum() > 50
    # AC12 / AC13 with altitude -1 (Q = 0) stored from positions only
    assert ((g["alt_all_none"] == -1) & (g["altset_all_none"] == 1)).any()
    # velocities of every sign, zero fields
    vel = ok & (tc == 19)
    assert set(st[vel].tolist()) == {1, 2}
    assert (g["vrate_all_none"][vel] < 0).any() and (g["vrate_all_none"][vel] > 0).any() and (g["vrate_all_none"][vel] == 0).any()
    # Conservative repairs: published bits that differ from the received ones, AP replies repaired into DF 17/18/19
    fixd = np.any(g["pfix_all_cons"] != 0, axis=1)
    assert fixd.sum() > 50
    assert (fixd & np.isin(df, (0, 4, 5, 16, 20, 21)) & np.isin(g["df_all_cons"], (17, 18, 19))).any()
    assert (fixd & np.isin(df, (11, 17, 19)) & (g["df_all_cons"] != df)).any()
    # a long sequence of a few aircraft
    assert np.bincount(g["seq"]).max() >= 900 and np.ptp(g["ts"][g["seq"] == g["seq"].max()]) > 180


# ---- the host function: a row and the incoming meta -> the reference's PDU -------------------------------------------------
TYPES = {0: type(None), 1: int, 2: float, 3: np.float64, 4: str}


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_decoded_pdu_equals_reference(g, tag, filt, corr):
    rows = expected(g, tag)
    vel = (rows["present"] & N.DEC_HAS_VELOCITY) != 0
    # the golden has speed / heading, the row integers: take them from the replay (checked above to give the same bits)
    rep = replay_rows(g, filt, corr)
    rows["velocity_we"], rows["velocity_sn"] = rep["velocity_we"], rep["velocity_sn"]
    names = ("callsign", "altitude", "speed", "heading", "vertical_rate", "latitude", "longitude", "num_msgs")
    n_dec = 0
    for i in range(len(rows)):
        meta = {"timestamp": float(g["ts"][i]), "snr": float(g["snr"][i])}
        out = N.decoded_pdu(rows[i], meta)
        port = int(g["port_" + tag][i])
        if port not in (1, 2):
            assert out is None
            continue
        name, (d, vec) = out
        assert name == ("decoded" if port == 1 else "unknown")
        assert np.array_equal(np.packbits(vec), g["bits"][i] ^ g["pfix_" + tag][i]) and vec.dtype == np.uint8
        assert tuple(d) == tuple(g["keys_decoded" if port == 1 else "keys_unknown"].tolist())
        assert d["datetime"] == str(g["datetime"][i]) and d["timestamp"] is meta["timestamp"] and d["snr"] is meta["snr"]
        assert d["df"] == int(g["df_" + tag][i]) and type(d["df"]) is int
        if port != 1:
            continue
        n_dec += 1
        assert d["icao"] == "{:06x}".format(int(g["icao_" + tag][i]))
        for k, name_ in enumerate(names):
            assert type(d[name_]) is TYPES[int(g["types_" + tag][i][k])], (i, name_, type(d[name_]))
        assert D.f64bits(d["speed"]) == int(g["speed_" + tag][i]) and D.f64bits(d["heading"]) == int(g["heading_" + tag][i])
        assert D.f64bits(d["latitude"]) == int(g["lat_" + tag][i]) and D.f64bits(d["longitude"]) == int(g["lon_" + tag][i])
        assert d["num_msgs"] == int(g["nmsgs_" + tag][i])
        if vel[i]:
            assert d["vertical_rate"] == int(g["vrate_" + tag][i])
    assert n_dec > 900


# ---- the emulated kernels ----------------------------------------------------------------------------------------------------
def dec_lib():
    srcs = [os.path.join(SIM_DIR, "decode_driver.cpp"), os.path.join(SIM_DIR, "sim_support.h"), os.path.join(SIM_DIR, "hipsim.h"),
            os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not (os.path.exists(DEC_SO) and all(os.path.getmtime(DEC_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", DEC_SO])
    return ctypes.CDLL(DEC_SO)


class SimDecoder:
    """One decoder of the emulated kernels: the aircraft table, its step state and the plane entries in host memory."""

    def __init__(self, lib, filt, corr):
        self.lib = lib
        self.table = np.full(1 << 24, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        self.planes = np.zeros((1 << 24) * lib.sim_dec_plane_bytes(), dtype=np.uint8)
        self.st = np.zeros(lib.sim_air_state_bytes(), dtype=np.uint8)
        self.next = 0
        self.epoch = 1
        self.fec = 1 if corr == "Conservative" else 0
        self.all = 1 if filt == "All Messages" else 0

    def reset(self):
        """A fresh decoder: the table emptied, the planes dropped by a new epoch (as adsb_reset does)."""
        self.table.fill(np.uint64(0xFFFFFFFFFFFFFFFF))
        self.st[:] = 0
        self.next = 0
        self.epoch += 1

    def call(self, bits14, ts, grid=4):
        b = np.ascontiguousarray(bits14, dtype=np.uint8).copy()
        t = np.ascontiguousarray(ts, dtype=np.float64)
        rows = np.zeros(len(b), dtype=N.DECODED_DTYPE)
        vp = ctypes.c_void_p
        rc = self.lib.sim_dec_pdus(b.ctypes.data_as(vp), t.ctypes.data_as(vp), ctypes.c_int(len(b)), ctypes.c_int(grid),
                              self.table.ctypes.data_as(vp), self.st.ctypes.data_as(vp), self.planes.ctypes.data_as(vp),
                              ctypes.c_uint(self.epoch), ctypes.c_ulonglong(self.next), ctypes.c_int(self.fec), ctypes.c_int(self.all),
                              rows.ctypes.data_as(vp))
        assert rc == 0, "the sort wrote outside its %d keys (-1) or left a key that names no record (-2): %d" % (len(b), rc)
        self.next += 1
        return rows


@pytest.fixture(scope="module")
def sim():
    lib = dec_lib()
    assert lib.sim_dec_row_bytes() == N.DECODED_DTYPE.itemsize
    return lib


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_emulated_kernels_one_pass(sim, g, tag, filt, corr):
    """Every golden sequence in one pass of its own decoder."""
    dec = SimDecoder(sim, filt, corr)
    got = np.zeros(len(g["bits"]), dtype=N.DECODED_DTYPE)
    for sl in seq_slices(g["seq"]):
        dec.reset()
        got[sl] = dec.call(g["bits"][sl], g["ts"][sl])
    check_rows(got, g, tag)


@pytest.mark.parametrize("tag,filt,corr", CONFIGS[:2])
def test_emulated_kernels_across_passes(sim, g, tag, filt, corr):
    """The long sequences cut into passes of 1-40 PDUs that share one table and one set of planes."""
    rng = np.random.default_rng(5)
    dec = SimDecoder(sim, filt, corr)
    sls = [sl for sl in seq_slices(g["seq"]) if sl.stop - sl.start >= 60]
    for sl in sls:
        dec.reset()
        got, i = [], sl.start
        while i < sl.stop:
            k = min(int(rng.integers(1, 41)), sl.stop - i)
            got.append(dec.call(g["bits"][i:i + k], g["ts"][i:i + k], grid=int(rng.integers(1, 4))))
            i += k
        check_rows(np.concatenate(got), g, tag, sl)


def test_emulated_kernels_many_aircraft_and_edge_addresses(sim):
    """Many aircraft in one pass, one aircraft with hundreds of records in a pass, addresses 0 and 0xFFFFFF: the emulated
    kernels equal the replay."""
    import decode_streams as S
    for filt, corr in (("All Messages", "None"), ("All Messages", "Conservative"), ("Extended Squitter Only", "None")):
        b14, ts = S.mixed(np.random.default_rng(11), n=3000, addresses=[0, 0xFFFFFF, 1, 0xFFFFFE] + list(range(0x400000, 0x400000 + 400)))
        b1, t1 = S.mixed(np.random.default_rng(12), n=600, addresses=[0xABCDEF], t0=float(ts[-1]) + 1)
        rep = D.Decoder(filt, corr)
        exp = rep.rows(np.concatenate([b14, b1]), np.concatenate([ts, t1]))
        dec = SimDecoder(sim, filt, corr)
        got = np.concatenate([dec.call(b14, ts), dec.call(b1, t1)])
        assert (got["present"] != 0).sum() > 2000
        assert got["num_msgs"].max() >= 300
        assert {0, 0xFFFFFF} <= set(got["icao"][got["present"] != 0].tolist())
        S.assert_rows_equal(got, exp)


SORT_TILE = 4096           # adsb_device.h kSortTile: the keys one workgroup of the sort takes
BUSY = 0x5A5A5A
_large = {}


def large_stream():
    """13500 PDUs in timestamp order: 7000 of one aircraft among 6500 of 3000 others, addresses 0 and 0xFFFFFF included."""
    import decode_streams as S
    if "stream" not in _large:
        others = [0, 0xFFFFFF, 1, 0xFFFFFE] + [0x300000 + 4099 * k for k in range(2996)]
        b0, t0 = S.mixed(np.random.default_rng(31), n=7000, addresses=[BUSY], dt=(0.002, 0.2))
        b1, t1 = S.mixed(np.random.default_rng(32), n=6500, addresses=others, dt=(0.002, 0.2))
        order = np.argsort(np.concatenate([t0, t1]), kind="stable")
        _large["stream"] = np.concatenate([b0, b1])[order], np.concatenate([t0, t1])[order]
    return _large["stream"]


def large_expected(filt, corr):
    """The replay's rows of large_stream in one decoder.  The busy aircraft's num_msgs counts its events, each of which has a
    sort key in a call that holds them all: more than a tile of them, so its sorted segment crosses a tile boundary wherever
    it starts."""
    import decode_streams as S
    if (filt, corr) not in _large:
        b14, ts = large_stream()
        exp = S.to_rows(D.Decoder(filt, corr).rows(b14, ts))
        assert len(exp) >= 10000 and exp["num_msgs"][exp["icao"] == BUSY].max() > SORT_TILE + 200
        planes = set(exp["icao"][(exp["present"] & N.DEC_HAS_PLANE) != 0].tolist())
        assert len(planes) > 2000 and {0, 0xFFFFFF} <= planes
        _large[(filt, corr)] = exp
    return _large[(filt, corr)]


LARGE_CONFIGS = (("All Messages", "None"), ("All Messages", "Conservative"), ("Extended Squitter Only", "None"))


@pytest.mark.parametrize("filt,corr", LARGE_CONFIGS)
def test_emulated_kernels_over_several_sort_tiles(sim, filt, corr):
    """More than three tiles of keys in one call, one aircraft's segment across a tile boundary; then the same stream in calls
    of a tile - 1, a tile, a tile + 1 and the rest on one decoder: both equal the replay."""
    import decode_streams as S
    b14, ts = large_stream()
    exp = large_expected(filt, corr)
    S.assert_rows_equal(SimDecoder(sim, filt, corr).call(b14, ts), exp)
    dec = SimDecoder(sim, filt, corr)
    cut = np.cumsum([0, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
    assert cut[-1] < len(b14)
    spans = list(zip(cut, list(cut[1:]) + [len(b14)]))
    S.assert_rows_equal(np.concatenate([dec.call(b14[lo:hi], ts[lo:hi]) for lo, hi in spans]), exp)


# ---- the NL zone edges on the CPR grid -----------------------------------------------------------------------------------------
EDGES = os.path.join(HERE, "golden", "g_decode_edges.npz")
GRID = 360.0 / 59 / 131072           # the coarser of the two latitude grids (odd frames); even frames: 6 / 131072


@pytest.fixture(scope="module")
def ge():
    return np.load(EDGES)


def test_edges_golden_holds_fixes_on_the_grid_points_beside_every_edge(ge):
    """From the reference's answers alone: beside each of the 58 edges, in both hemispheres, fixes on the last grid point below
    and the first at or above it, from an even and from an odd frame; pairs across an edge without a fix whose altitude is
    stored; NL = 1, latitude 0, longitudes on each side of 180, latitudes on each side of the 270 wrap, negative j and m."""
    lat, lon = ge["lat_all_none"].view(np.float64), ge["lon_all_none"].view(np.float64)
    fix = ~np.isnan(lat)
    for e in D.NL_EDGES:
        for sign in (1, -1):
            a = sign * lat[fix & (np.sign(lat) == sign)]
            below, above = np.unique(a[(a >= e - GRID) & (a < e)]), np.unique(a[(a >= e) & (a < e + GRID)])
            assert len(below) >= 2 and len(above) >= 2, (e, sign, below, above)
    bits = np.unpackbits(ge["bits"], axis=1)
    fld = lambda lo, n: bits[:, lo:lo + n].dot(1 << np.arange(n - 1, -1, -1))      # noqa: E731
    sls = seq_slices(ge["seq"])
    nofix = [sl for sl in sls if not fix[sl].any()]
    assert len(nofix) >= 2 * 2 * 58 and all((ge["altset_all_none"][sl] == 1).all() for sl in nofix)
    assert (fix & (np.abs(lat) >= 87) & (np.abs(lat) <= 90)).sum() >= 20 and (fix & (lat == 0)).any()
    assert (fix & (lon > 179.999)).any() and (fix & (lon < -179.999)).any()
    assert (fix & (lat > 269.99)).any() and (fix & (lat < -89.999)).any()
    odd, clat, clon = fld(53, 1), fld(54, 17), fld(71, 17)
    js, ms = [], []
    for sl in sls:
        i = sl.start
        assert (odd[i], odd[i + 1], odd[i + 2]) == (0, 1, 0) and sl.stop - i == 3
        js.append(np.floor(59 * clat[i] / 131072 - 60 * clat[i + 1] / 131072 + 0.5))
        if fix[i + 1]:
            n = D.nl(lat[i + 1])
            ms.append(np.floor(clon[i] / 131072 * (n - 1) - clon[i + 1] / 131072 * n + 0.5))
    assert min(js) < 0 < max(js) and min(ms) < 0 < max(ms)


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_replay_equals_edges_golden(ge, tag, filt, corr):
    check_rows(replay_rows(ge, filt, corr), ge, tag)


@pytest.mark.parametrize("tag,filt,corr", CONFIGS[:1] + CONFIGS[3:])
def test_emulated_kernels_equal_edges_golden(sim, ge, tag, filt, corr):
    """The sequences use distinct addresses: one decoder takes them all in one call, as many aircraft at once."""
    assert len(set(ge["icao_all_none"].tolist())) == len(seq_slices(ge["seq"]))
    check_rows(SimDecoder(sim, filt, corr).call(ge["bits"], ge["ts"]), ge, tag)


# ---- resources ---------------------------------------------------------------------------------------------------------------
def test_kernel_resources_fit_beside_every_k_detect():
    """The decode step runs behind the table step, beside the next pass's k_detect: no scratch, no spills, LDS and VGPRs that
    leave room for a workgroup beside every k_detect instance (the check of tests/test_aircraft.py).  The sort is the
    library's own (k_dec_sort_*): no library kernels."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    LDS_CU, VGPR_SIMD, SIMDS, GRAN = 160 * 1024, 512, 4, 1280
    alloc = lambda v: -(-v // 8) * 8                                    # noqa: E731
    gran = lambda b: -(-b // GRAN) * GRAN                               # noqa: E731
    dec = {k: v for k, v in res.items() if "k_dec" in k}
    assert len(dec) == 6, sorted(dec)      # classify, fold, pdu_flags, sort_hist, sort_scan, sort_scatter
    assert not [k for k in res if "rocprim" in k or "cub" in k]
    detect = {k: v for k, v in res.items() if "k_detect" in k}
    assert len(detect) == 35
    for name, d in detect.items():
        mode = int(re.search(r"k_detectILi(\d)E", name).group(1))
        wpb = 1 if mode in (3, 4, 5, 6) else 4
        wg_cu = min(LDS_CU // gran(d["lds_bytes_per_block"]), SIMDS * (VGPR_SIMD // alloc(d["vgprs"])) // wpb, 32)
        free_lds = LDS_CU - wg_cu * gran(d["lds_bytes_per_block"])
        per_simd = [6, 5, 5, 5] if wpb == 1 else [5, 5, 5, 5]
        for fname, f in dec.items():
            assert f["scratch_bytes_per_lane"] == 0 and f["vgpr_spills"] == 0 and f["sgpr_spills"] == 0, fname
            assert gran(f["lds_bytes_per_block"]) <= free_lds, (fname, name)
            slots = sum((VGPR_SIMD - w * alloc(d["vgprs"])) // alloc(f["vgprs"]) for w in per_simd)
            assert slots >= 4, (fname, f["vgprs"], name, d["vgprs"])


def test_flag_and_abi_constants():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_FLAG_DECODE 512u", src)
    assert N.FLAG_DECODE == 512 and N.ABI_VERSION == 5
    for name in ("adsb_set_decoder", "adsb_last_decoded", "adsb_decode_pdus"):
        assert name in N.EXPORTS and name in src
