"""Plane snapshots on the CPU (adsb_planes / adsb_stream_planes): the emulated k_planes_* kernels (tests/sim/planes_driver.cpp,
over the decoders of decode_driver.cpp and fleet_driver.cpp) against tests/golden/g_planes.npz -- the reference decoder's final
plane_dict and the lines its print_planes draws -- and against the plain-Python replay (tests/decode_replay.py); the host
functions _native.plane_entry / plane_table, the declared symbols and the kernels' resources.

What a green run here does NOT cover: the driver restates the host's argument rules and launch order (adsb_hip.hip adsb_planes /
adsb_stream_planes); the host code itself runs in tests/test_gpu_planes.py only.

One entry of the reference has no counterpart: under "Conservative" a repaired reply can be filed under the address ""
(decoder.py: update_plane(self.aa_str) with an empty aa_str); the device files such a PDU under no address (icao -1 in its
row, tests/golden/g_decode.npz the same) and keeps no plane for it.  The golden records that entry with icao -1; it is left
out of every comparison here."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import decode_replay as D
import decode_streams as S
import test_decode as TD
import test_stream_decode as TS
from gr_adsb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
PLANES_SO = os.path.join(SIM_DIR, "libadsb_planes_sim.so")
GOLD = os.path.join(HERE, "golden", "g_planes.npz")
CONFIGS = TD.CONFIGS
NAN_BITS = TD.NAN_BITS
CHUNK = 2048                 # adsb_device.h kPlanesChunk: the addresses one wavefront scans
TOP = 1 << 24
ENOSPC, EINVAL = -28, -22
# adsb_device.h Plane, for the states fabricated below
PLANE_DTYPE = np.dtype([("epoch", "<u4"), ("num_msgs", "<u4"), ("present", "<u4"), ("altitude", "<i4"), ("callsign", "S8"),
                        ("vwe", "<i4"), ("vsn", "<i4"), ("vr", "<i4"), ("cpr", "<i4", (4,)), ("pad", "<i4"), ("cpr_t", "<i8", (2,)),
                        ("lat", "<f8"), ("lon", "<f8")])
FIELDS = ("callsign", "altitude", "speed", "heading", "vertical_rate", "latitude", "longitude", "num_msgs")


@pytest.fixture(scope="module")
def sim():
    srcs = [os.path.join(SIM_DIR, f) for f in ("planes_driver.cpp", "fleet_driver.cpp", "decode_driver.cpp", "sim_support.h", "hipsim.h")] + \
        [os.path.join(HERE, "..", "gr_adsb_amd", "csrc", "adsb_device.h")]
    if not (os.path.exists(PLANES_SO) and all(os.path.getmtime(PLANES_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", PLANES_SO])
    lib = ctypes.CDLL(PLANES_SO)
    lib.sim_fleet_open.restype = ctypes.c_void_p
    lib.sim_fleet_taken.restype = ctypes.c_longlong
    lib.sim_fleet_gen_max.restype = ctypes.c_uint
    assert lib.sim_planes_chunk() == CHUNK and TOP % CHUNK == 0
    assert lib.sim_dec_row_bytes() == N.DECODED_DTYPE.itemsize and lib.sim_dec_plane_bytes() == PLANE_DTYPE.itemsize == 88
    return lib


@pytest.fixture(scope="module")
def g():
    return np.load(TD.GOLD)


@pytest.fixture(scope="module")
def gp():
    return np.load(GOLD)


# ---- expectations ------------------------------------------------------------------------------------------------------------
def plane_rows(planes):
    """decode_replay.Decoder.planes -> the snapshot's rows (ascending address)."""
    out = np.zeros(len(planes), dtype=N.DECODED_DTYPE)
    for i, a in enumerate(sorted(planes)):
        p = planes[a]
        pr = N.DEC_HAS_PLANE | (N.DEC_HAS_CALLSIGN if p["callsign"] is not None else 0) | \
            (N.DEC_HAS_ALTITUDE if p["altitude"] is not None else 0) | (N.DEC_HAS_VELOCITY if p["vel"] is not None else 0)
        vel = p["vel"] or (0, 0, 0)
        out[i] = (0, 0, pr, 0, a, np.zeros(14, np.uint8), (p["callsign"] or "").encode(), (0, 0), p["altitude"] or 0, vel[0], vel[1],
                  vel[2], p["lat"], p["lon"], p["n"], 0)
    return out


def rows_equal(got, exp):
    """DECODED_DTYPE rows byte for byte; empty arrays are equal."""
    assert len(got) == len(exp), (len(got), len(exp))
    if len(got):
        S.assert_rows_equal(got, exp)


def golden_of(gp, tag, seq):
    """The golden's entries of one sequence, ascending address, the "" entry left out: a dict of arrays."""
    m = np.flatnonzero((gp["seq_" + tag] == seq) & (gp["icao_" + tag] >= 0))
    m = m[np.argsort(gp["icao_" + tag][m], kind="stable")]
    return {k: gp["%s_%s" % (k, tag)][m] for k in ("icao", "cs", "csset", "alt", "altset", "speed", "heading", "vrate", "vrset", "lat",
                                                  "lon", "nmsgs", "types", "line")}


def check_against_golden(rows, e, what):
    """Snapshot rows against golden_of's entries: float64 fields by their bits, speed / heading from the integer components."""
    assert len(rows) == len(e["icao"]), (what, len(rows), len(e["icao"]))
    if not len(rows):
        return
    assert np.array_equal(rows["icao"], e["icao"]), what
    vel = e["speed"] != NAN_BITS
    assert np.array_equal(vel, e["vrset"] == 1)
    present = N.DEC_HAS_PLANE | (e["csset"] * N.DEC_HAS_CALLSIGN) | (e["altset"] * N.DEC_HAS_ALTITUDE) | (vel * N.DEC_HAS_VELOCITY)
    assert np.array_equal(rows["present"], present), what
    assert [bytes(c).rstrip(b"\0") for c in e["cs"]] == [bytes(c) for c in rows["callsign"]], what
    assert np.array_equal(rows["altitude"], e["alt"]) and np.array_equal(rows["vertical_rate"], e["vrate"]), what
    assert np.array_equal(rows["num_msgs"], e["nmsgs"]), what
    assert np.array_equal(rows["latitude"].view(np.uint64), e["lat"]) and np.array_equal(rows["longitude"].view(np.uint64), e["lon"]), what
    for i in np.flatnonzero(vel):
        s, h = D.speed_heading(int(rows["velocity_we"][i]), int(rows["velocity_sn"][i]))
        assert D.f64bits(s) == int(e["speed"][i]) and D.f64bits(h) == int(e["heading"][i]), what
    assert not rows["port"].any() and not rows["df"].any() and not rows["bits"].any()
    assert not rows["pad0"].any() and not rows["pad1"].any() and not rows["pad2"].any()


def windows(addresses):
    """Chunk-aligned address ranges that cover the given addresses, the first and the last chunk: [(lo, hi)], ascending, merged."""
    chunks = sorted({int(a) // CHUNK for a in addresses} | {0, TOP // CHUNK - 1})
    out = []
    for c in chunks:
        if out and out[-1][1] == c * CHUNK:
            out[-1][1] = (c + 1) * CHUNK
        else:
            out.append([c * CHUNK, (c + 1) * CHUNK])
    return [tuple(w) for w in out]


def dense(lib, dec, lo=0, hi=TOP, cap=None, grid=3):
    """adsb_planes on a test_decode.SimDecoder over [lo, hi): (rc, n, rows[:min(n, cap)]).  cap None: a count query first."""
    vp = ctypes.c_void_p
    n = ctypes.c_int(-1)

    def call(k):
        rows = np.zeros(k, dtype=N.DECODED_DTYPE)
        rc = lib.sim_planes_dense(dec.table.ctypes.data_as(vp), dec.planes.ctypes.data_as(vp), ctypes.c_uint(dec.epoch), ctypes.c_uint(lo),
                                  ctypes.c_uint(hi), ctypes.c_int(grid), ctypes.c_int(k), rows.ctypes.data_as(vp), ctypes.byref(n))
        assert rc in (0, ENOSPC), "a kernel wrote behind its arrays (-1) or a bad range (-22): %d" % rc
        return rc, rows
    if cap is None:
        rc, _ = call(0)
        assert rc == (ENOSPC if n.value else 0)
        cap = n.value
    rc, rows = call(cap)
    return rc, n.value, rows[:min(n.value, cap)]


def dense_over(lib, dec, addresses):
    """The snapshot over windows(addresses), concatenated.  Every plane has one of the addresses, so that many rows are room
    enough (or the call says so); one workgroup: a window is seldom more than one chunk."""
    parts = []
    for lo, hi in windows(addresses):
        rc, n, rows = dense(lib, dec, lo, hi, cap=len(set(addresses)), grid=1)
        assert rc == 0 and n == len(rows)
        parts.append(rows)
    return np.concatenate(parts)


# ---- the golden itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_golden_entries_equal_the_last_row_of_their_address(g, gp, tag, filt, corr):
    """No reference needed: an address's final plane_dict entry is what g_decode.npz's last row with a plane shows for it."""
    rows = TD.expected(g, tag)
    n_planes = 0
    for seq, sl in enumerate(TD.seq_slices(g["seq"])):
        e = golden_of(gp, tag, seq)
        r = rows[sl]
        has = (r["present"] & N.DEC_HAS_PLANE) != 0
        assert set(e["icao"].tolist()) == set(r["icao"][has].tolist())
        for i, a in enumerate(e["icao"]):
            k = sl.start + int(np.flatnonzero(has & (r["icao"] == a))[-1])
            assert rows["num_msgs"][k] == e["nmsgs"][i] and rows["altitude"][k] == e["alt"][i]
            assert bytes(rows["callsign"][k]) == bytes(e["cs"][i]).rstrip(b"\0")
            assert int(g["speed_" + tag][k]) == int(e["speed"][i]) and int(g["heading_" + tag][k]) == int(e["heading"][i])
            assert int(g["lat_" + tag][k]) == int(e["lat"][i]) and int(g["lon_" + tag][k]) == int(e["lon"][i])
            assert int(g["vrate_" + tag][k]) == int(e["vrate"][i]) and int(g["csset_" + tag][k]) == int(e["csset"][i])
            assert int(g["altset_" + tag][k]) == int(e["altset"][i])
            n_planes += 1
    assert n_planes >= 190
    assert tuple(gp["keys"].tolist()) == FIELDS[:7] + ("cpr", "num_msgs", "last_seen")
    # the entry under "" (module docstring): only where the repair runs under "All Messages"
    assert int((gp["icao_" + tag] < 0).sum()) == (3 if tag == "all_cons" else 0)


# ---- one decoder on the emulated kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_dense_snapshot_equals_golden_and_replay(sim, g, gp, tag, filt, corr):
    """Every golden sequence decoded by the emulated kernels in a decoder of its own: the snapshot (over the chunks of every
    address the sequence names, the first and the last chunk) equals the reference's plane_dict and the replay's planes."""
    dec = TD.SimDecoder(sim, filt, corr)
    total = 0
    for seq, sl in enumerate(TD.seq_slices(g["seq"])):
        dec.reset()
        got = dec.call(g["bits"][sl], g["ts"][sl])
        rep = D.Decoder(filt, corr)
        rep.rows(g["bits"][sl], g["ts"][sl])
        snap = dense_over(sim, dec, [a for a in got["icao"] if a >= 0])
        check_against_golden(snap, golden_of(gp, tag, seq), (tag, seq))
        rows_equal(snap, plane_rows(rep.planes))
        total += len(snap)
    assert total >= 190


def ident(aa, rng):
    """An identification squitter of aircraft aa: always a plane."""
    body = np.zeros(51, np.uint8)
    for k in range(8):
        body[3 + 6 * k:9 + 6 * k] = S.ib(int(rng.integers(1, 27)), 6)
    return np.packbits(S.es(aa, int(rng.integers(1, 5)), body))


EDGE = [0, 1, 0xFFFFFE, 0xFFFFFF, CHUNK - 1, CHUNK, TOP - CHUNK - 1, TOP - CHUNK]


def test_dense_snapshot_of_the_whole_address_space(sim):
    """Addresses 0, 1, 0xFFFFFE, 0xFFFFFF and the pairs that straddle the first and the last chunk boundary among 300 others,
    scanned from 0 to 2^24 by a grid that does not divide the chunks; one chunk short of room (cap = needed - 1) gives the
    count and the first cap rows; a second snapshot is identical; 600 PDUs more and the snapshot is the replay's again."""
    addr = EDGE + [0x400000 + 523 * k for k in range(300)]
    b, t = S.mixed(np.random.default_rng(41), n=2500, addresses=addr)
    for filt, corr in (("All Messages", "Conservative"),):
        dec, rep = TD.SimDecoder(sim, filt, corr), D.Decoder(filt, corr)
        rows_equal(dec.call(b, t), rep.rows(b, t))
        exp = plane_rows(rep.planes)
        assert set(EDGE) <= set(exp["icao"].tolist()) and len(exp) > 250
        rc, n, rows = dense(sim, dec, grid=5)
        assert rc == 0 and n == len(exp)
        rows_equal(rows, exp)
        rc, n, part = dense(sim, dec, cap=len(exp) - 1, grid=5)
        assert rc == ENOSPC and n == len(exp)
        rows_equal(part, exp[:-1])
        rows_equal(dense_over(sim, dec, addr), exp)          # (a second snapshot, by windows)
        b1, t1 = S.mixed(np.random.default_rng(42), n=600, addresses=addr[::3] + [0x123456], t0=float(t[-1]) + 1)
        rows_equal(dec.call(b1, t1), rep.rows(b1, t1))       # rows decoded after a snapshot: the replay's, unchanged
        later = plane_rows(rep.planes)
        assert len(later) == len(exp) + 1 and (later["num_msgs"].sum() > exp["num_msgs"].sum())
        rows_equal(dense_over(sim, dec, addr + [0x123456]), later)


def test_dense_snapshot_of_a_full_chunk_beside_an_empty_one(sim):
    """Every address of chunk 2 live, chunks 1 and 3 empty: 2048 rows in address order, whatever the grid."""
    rng = np.random.default_rng(43)
    addr = list(range(2 * CHUNK, 3 * CHUNK))
    b = np.array([ident(a, rng) for a in addr], np.uint8)
    t = 1760000000.5 + 0.01 * np.arange(len(addr))
    dec, rep = TD.SimDecoder(sim, "Extended Squitter Only", "None"), D.Decoder("Extended Squitter Only", "None")
    rows_equal(dec.call(b, t), rep.rows(b, t))
    exp = plane_rows(rep.planes)
    assert len(exp) == CHUNK
    for grid in (1, 2):
        rc, n, rows = dense(sim, dec, CHUNK, 4 * CHUNK, grid=grid)
        assert rc == 0 and n == CHUNK
        rows_equal(rows, exp)
    for lo, hi in ((CHUNK, 2 * CHUNK), (3 * CHUNK, 4 * CHUNK), (0, 2 * CHUNK)):
        assert dense(sim, dec, lo, hi)[:2] == (0, 0)
    rc, n, rows = dense(sim, dec, 2 * CHUNK, 2 * CHUNK + 10)             # a range that ends inside a chunk
    assert (rc, n) == (0, 10)
    rows_equal(rows, exp[:10])


def test_dense_snapshot_of_nothing_of_a_reset_and_of_an_announced_address(sim):
    """An empty table; after a reset (a new epoch, the old entries still in memory); a table entry without a plane and a stale
    plane under a fresh table entry, both fabricated in the decoder's host memory: none of them is a plane."""
    dec = TD.SimDecoder(sim, "All Messages", "None")
    assert dense(sim, dec, 0, 4 * CHUNK)[:2] == (0, 0)
    addr = [0, 5, CHUNK - 1, CHUNK, 3000]
    b, t = S.mixed(np.random.default_rng(44), n=200, addresses=addr)
    rep = D.Decoder("All Messages", "None")
    rows_equal(dec.call(b, t), rep.rows(b, t))
    exp = plane_rows(rep.planes)
    assert len(exp) == len(addr)
    rows_equal(dense(sim, dec, 0, 4 * CHUNK)[2], exp)
    planes = dec.planes.view(PLANE_DTYPE)
    dec.table[7] = 12345                      # announced (a DF 11 the msg_filter rejected, say): no plane
    assert planes[7]["present"] == 0
    rows_equal(dense(sim, dec, 0, 4 * CHUNK)[2], exp)
    dec.reset()
    assert (planes[addr]["present"] & N.DEC_HAS_PLANE).all() and (planes[addr]["epoch"] == dec.epoch - 1).all()
    assert dense(sim, dec, 0, 4 * CHUNK)[:2] == (0, 0)
    dec.table[5] = 0                          # heard again in the new epoch, before any plane: the stale entry stays out
    assert dense(sim, dec, 0, 4 * CHUNK)[:2] == (0, 0)
    planes["epoch"][5] = dec.epoch            # ... and is a plane once its epoch is the current one
    rc, n, rows = dense(sim, dec, 0, 4 * CHUNK)
    assert (rc, n) == (0, 1) and rows["icao"][0] == 5
    rows_equal(rows, exp[exp["icao"] == 5])


# ---- the fleet on the emulated kernels ---------------------------------------------------------------------------------------
def fleet(lib, f, streams=None, cap=None, grid=3, want_first=True):
    """adsb_stream_planes on a test_stream_decode.SimFleet: (rc, n, rows, first)."""
    vp = ctypes.c_void_p
    n = ctypes.c_int(-1)
    sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
    k = 0 if sel is None else len(sel)
    nf = (f.n_streams if sel is None else k) + 1
    first = np.full(nf, -7, dtype=np.int32)

    def call(c_):
        rows = np.zeros(c_, dtype=N.DECODED_DTYPE)
        rc = lib.sim_planes_fleet(f.h, None if sel is None else sel.ctypes.data_as(vp), ctypes.c_int(k), ctypes.c_int(grid), ctypes.c_int(c_),
                                  rows.ctypes.data_as(vp), first.ctypes.data_as(vp) if want_first else None, ctypes.byref(n))
        assert rc in (0, ENOSPC, EINVAL), "a kernel wrote behind its arrays (-1), error word / unsorted keys (-3): %d" % rc
        return rc, rows
    if cap is None:
        rc, _ = call(0)
        if rc == EINVAL:
            return rc, -1, None, None
        assert rc == (ENOSPC if n.value else 0)
        cap = n.value
    rc, rows = call(cap)
    return rc, n.value, rows[:min(max(n.value, 0), cap)], first


def open_fleet(lib, n_streams, filt, corr, **kw):
    f = TS.SimFleet(lib, n_streams, filt, corr, **kw)
    f.n_streams = n_streams
    return f


def check_fleet(lib, f, rep, streams=None, grid=3):
    """The snapshot of `streams` against the replays' planes, stream by stream; returns the rows."""
    rc, n, rows, first = fleet(lib, f, streams, grid=grid)
    ids = list(range(f.n_streams)) if streams is None else list(streams)
    assert rc == 0 and first[0] == 0 and first[-1] == n == len(rows) and np.all(np.diff(first) >= 0)
    for i, s in enumerate(ids):
        rows_equal(rows[first[i]:first[i + 1]], plane_rows(rep.dec[s].planes))
    return rows


SHARED = [0, 0xFFFFFF] + [0x480000 + 977 * k for k in range(148)]
_shared = {}


def shared_fleet(lib):
    """40 streams: 1 .. 37 hear the same 150 aircraft, 0, 38 and 39 nothing.  (fleet, replays), decoded once."""
    if "f" not in _shared:
        filt, corr = "All Messages", "Conservative"
        tr = [S.mixed(np.random.default_rng(300 + s), n=260, addresses=SHARED, t0=1760000000.5 + 0.37 * s, dt=(0.002, 0.05))
              for s in range(37)]
        b, t, s = TS.interleave(tr)
        s = s + 1
        f, rep = open_fleet(lib, 40, filt, corr), TS.Replays(40, filt, corr)
        rng = np.random.default_rng(45)
        for lo, hi in TS.cuts(rng, len(b), 1500, 4000):
            rows_equal(f.call(b[lo:hi], t[lo:hi], s[lo:hi]), rep.call(b[lo:hi], t[lo:hi], s[lo:hi]))
        assert f.stats()["planes"] == rep.planes() > TS.SORT_TILE
        _shared["f"] = f, rep
    return _shared["f"]


def test_fleet_snapshot_of_streams_that_share_their_aircraft(sim):
    """Every stream's rows are its own replay's planes, (stream, address) order, more than a sort tile of keys in all; streams
    without planes -- the first and the last two -- are empty ranges; two snapshots are identical; first may be left out."""
    f, rep = shared_fleet(sim)
    rows = check_fleet(sim, f, rep)
    assert len(rows) > TS.SORT_TILE
    rc, n, rows2, first = fleet(sim, f, grid=2)
    assert rows.tobytes() == rows2.tobytes()
    assert first[0] == first[1] == 0 and first[38] == first[39] == first[40] == n
    rc, n3, rows3, first3 = fleet(sim, f, want_first=False)
    assert rc == 0 and rows3.tobytes() == rows.tobytes() and (first3 == -7).all()
    # one row short
    rc, n4, _, _ = fleet(sim, f, cap=n - 1)
    assert rc == ENOSPC and n4 == n


def test_fleet_snapshot_of_a_selection(sim):
    """A single stream, the first plus the last, a few in between: the matching ranges of the full snapshot."""
    f, rep = shared_fleet(sim)
    full = check_fleet(sim, f, rep)
    _, _, _, ffirst = fleet(sim, f)
    for sel in ([17], [0], [39], [0, 39], [1, 37], [0, 5, 6, 30, 39], []):
        rows = check_fleet(sim, f, rep, streams=sel)
        assert rows.tobytes() == b"".join(full[ffirst[s]:ffirst[s + 1]].tobytes() for s in sel)


@pytest.mark.parametrize("sel", ([3, 3], [5, 2], [-1, 4], [0, 40], [40], [1, 2, 2]))
def test_a_bad_selection_is_refused(sim, sel):
    """The host's rule for a selection (adsb_stream_planes: -EINVAL), as the driver restates it and as _native checks it before
    the call."""
    f, _ = shared_fleet(sim)
    assert fleet(sim, f, streams=sel)[0] == EINVAL
    with pytest.raises(ValueError):
        N.check_stream_selection(sel, 40)
    N.check_stream_selection([0, 39], 40)
    N.check_stream_selection([], 40)


def test_fleet_snapshot_after_a_reset_a_rehash_and_a_growth(sim):
    """A store of 256 slots: a reset stream is empty at once while its slots are still taken; a rehash (forced by a reset at
    the last generation) and a growth (forced by a call of noise) leave the snapshot's bytes as they were.  One stream's
    generation starts just below the largest (the test hook of the driver)."""
    filt, corr = "All Messages", "None"
    gen_max = int(sim.sim_fleet_gen_max())
    f, rep = open_fleet(sim, 5, filt, corr, slots=0), TS.Replays(5, filt, corr)
    f.set_gen(3, gen_max - 1)
    f.set_gen(4, gen_max)
    addr = [0, 0xFFFFFF] + [0x500000 + 4099 * k for k in range(18)]
    b, t, s = TS.interleave([S.mixed(np.random.default_rng(400 + k), n=28, addresses=addr, t0=1760000100.25 + 0.11 * k, dt=(0.002, 0.05))
                             for k in range(4)])
    rows_equal(f.call(b, t, s), rep.call(b, t, s))
    assert f.stats()["capacity"] == 256 and f.stats()["grows"] == 0 and rep.planes() > 40
    before = check_fleet(sim, f, rep)
    # a reset: gone from the snapshot, not from the store
    taken = f.taken()
    f.reset(1)
    rep.reset(1)
    assert f.taken() == taken and f.stats()["planes"] == rep.planes()
    after = check_fleet(sim, f, rep)
    assert len(after) < len(before) and len(check_fleet(sim, f, rep, streams=[1])) == 0
    # stream 3 at the last generation, heard again
    f.reset(3)
    rep.reset(3)
    b1, t1 = S.mixed(np.random.default_rng(410), n=40, addresses=addr[:9], t0=float(t[-1]) + 1)
    s1 = np.full(len(b1), 3, np.int32)
    rows_equal(f.call(b1, t1, s1), rep.call(b1, t1, s1))
    snap = check_fleet(sim, f, rep)
    # a rehash: the empty stream 4 leaves its last generation
    taken = f.taken()
    f.reset(4)
    assert f.taken() < taken and f.stats()["capacity"] == 256
    assert check_fleet(sim, f, rep).tobytes() == snap.tobytes()
    # a growth: 200 rows of noise need room the store does not have
    noise = np.random.default_rng(411).integers(0, 256, (200, 14)).astype(np.uint8)
    tn = float(t1[-1]) + 1 + 0.01 * np.arange(200)
    sn = np.zeros(200, np.int32)
    planes = rep.planes()
    rows_equal(f.call(noise, tn, sn), rep.call(noise, tn, sn))
    assert rep.planes() == planes and f.stats()["grows"] == 1 and f.stats()["capacity"] > 256
    assert check_fleet(sim, f, rep).tobytes() == snap.tobytes()
    # the last generation used up: stream 3 wraps through a rehash and is empty
    f.reset(3)
    rep.reset(3)
    assert len(check_fleet(sim, f, rep, streams=[3])) == 0
    check_fleet(sim, f, rep)
    f.close()


def test_fleet_snapshot_of_five_thousand_planes(sim):
    """5000 planes over 40 streams in one snapshot: the key sort runs over two tiles."""
    rng = np.random.default_rng(46)
    addr = [0, 0xFFFFFF] + [0x600000 + 8191 * k for k in range(123)]
    b = np.array([ident(a, rng) for _ in range(40) for a in addr], np.uint8)
    s = np.repeat(np.arange(40, dtype=np.int32), len(addr))
    t = 1760000200.5 + 0.001 * np.arange(len(b))
    f, rep = open_fleet(sim, 40, "Extended Squitter Only", "None"), TS.Replays(40, "Extended Squitter Only", "None")
    rows_equal(f.call(b, t, s), rep.call(b, t, s))
    rows = check_fleet(sim, f, rep, grid=4)
    assert len(rows) == 5000 > TS.SORT_TILE
    f.close()


# ---- host only ---------------------------------------------------------------------------------------------------------------
TYPES = {0: type(None), 1: int, 2: float, 3: np.float64, 4: str}


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_plane_entry_and_plane_table_equal_the_reference(g, gp, tag, filt, corr):
    """_native.plane_entry of the replay's rows (shown above to be the snapshot's) has the reference entry's keys, Python types
    and values; _native.plane_table draws print_planes' lines (the reference's in its order of first hearing, these by address)."""
    n = 0
    for seq, sl in enumerate(TD.seq_slices(g["seq"])):
        rep = D.Decoder(filt, corr)
        rep.rows(g["bits"][sl], g["ts"][sl])
        rows = plane_rows(rep.planes)
        e = golden_of(gp, tag, seq)
        check_against_golden(rows, e, (tag, seq))
        for i, row in enumerate(rows):
            d = N.plane_entry(row)
            assert tuple(d) == FIELDS
            for k, name in enumerate(FIELDS):
                assert type(d[name]) is TYPES[int(e["types"][i][k])], (tag, seq, name, type(d[name]))
            assert d["callsign"] == (bytes(e["cs"][i]).rstrip(b"\0").decode() if e["csset"][i] else None)
            for name, key in (("speed", "speed"), ("heading", "heading"), ("latitude", "lat"), ("longitude", "lon")):
                assert D.f64bits(d[name]) == int(e[key][i]), (tag, seq, name)
            assert d["num_msgs"] == int(e["nmsgs"][i])
            assert (d["altitude"] == int(e["alt"][i])) if e["altset"][i] else np.isnan(d["altitude"])
            assert (d["vertical_rate"] == int(e["vrate"][i])) if e["vrset"][i] else np.isnan(d["vertical_rate"])
            n += 1
        assert N.plane_table(rows, float(g["ts"][sl.stop - 1])) == [str(x) for x in e["line"]]
    assert n >= 190


def test_exports_and_abi_constants():
    src = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert len(re.findall(r"^int adsb_(stream_)?planes\(adsb_ctx\* ctx", src, re.M)) == 2
    assert re.search(r"^int adsb_planes\(adsb_ctx\* ctx", src, re.M) and re.search(r"^int adsb_stream_planes\(adsb_ctx\* ctx", src, re.M)
    assert "adsb_planes" in N.EXPORTS and "adsb_stream_planes" in N.EXPORTS
    assert N.ABI_VERSION == 5 and re.search(r"#define ADSB_ABI_VERSION 5\b", src)
    assert "last_seen" in src[src.index("PLANE SNAPSHOTS"):src.index("int adsb_planes(")]


def test_snapshot_kernels_have_no_scratch_and_no_spills(capsys):
    """Four new kernels, none of whose names falls under another test's selection; their resources as the compiler reports them
    (printed).  They run alone on the context's stream, not beside k_detect: no co-residency bound applies."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES))
    ks = {k: v for k, v in res.items() if "k_planes_" in k}
    names = sorted(re.search(r"k_planes_[a-z_]+?(?=E)", k).group(0) for k in ks)
    assert names == ["k_planes_emit", "k_planes_store_emit", "k_planes_store_keys", "k_planes_tally"], sorted(ks)
    for k, v in ks.items():
        with capsys.disabled():
            print("\n%s: %d VGPRs, %d SGPRs, %d B LDS, occupancy %d" % (k, v["vgprs"], v["sgprs"], v["lds_bytes_per_block"],
                                                                         v["occupancy_waves_per_simd"]), end="")
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, k
        assert not any(t in k for t in ("k_fleet", "k_stream_", "k_dec", "k_air", "k_fec", "k_batch", "k_detect", "k_order",
                                        "k_resolve", "k_count", "k_compact", "rocprim", "cub")), k
