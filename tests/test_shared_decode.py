"""ADSB_FLAG_STREAM_DECODE_SHARED on the CPU: one decoder behind all receiver streams, fed every call's records in the order
ascending (timestamp, list position).  The emulated kernels (tests/sim/shared_driver.cpp: adsb_shared_device.h's time order
around the k_fleet_* decode step, the host's growth rule restated) against tests/golden/g_shared.npz -- ONE unmodified
reference decoder fed the merged sequence (tools/make_golden_shared.py) -- and against the plain-Python replays over the same
sequence; the pair sort alone; the new translation unit's build facts.

What a green run here does NOT cover: the host's own shared branch of fleet_step, the entry points and the plane calls on a
shared context -- tests/test_gpu_shared_decode.py; and everything on the device's side of these seams: what hipcc makes of
k_shared_sort_scatter's ballots and k_shared_sort_scan's __shfl_up scan with its carry, the real launchers' grid sizing (the
launches here are the driver's own) and the kernels' second grid-stride round under them, which k_shared_scatter reaches at
58 255 records and the others above 524 288 -- tests/test_gpu_shared_device.py runs this file's sort cases, unchanged, on the
MI355X through tests/gpu/shared_device_driver.hip, and adds the chain keys -> sort -> gather -> scatter at both sizes."""
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
from gr_adsb_amd import _native as N
from shared_replay import GOLD, Replay, golden_calls, rows_of, time_order

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
SHARED_SO = os.path.join(SIM_DIR, "libadsb_shared_sim.so")
CONFIGS = TD.CONFIGS
SORT_TILE = 4096
MIN_CAP = 256
AP_BITS = N.BURST_AP_KNOWN | N.BURST_AP_FEC
vp = ctypes.c_void_p


def shared_lib():
    csrc = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, f) for f in ("shared_driver.cpp", "fleet_driver.cpp", "sim_support.h", "hipsim.h")] + \
        [os.path.join(csrc, "adsb_device.h"), os.path.join(csrc, "adsb_shared_device.h")]
    if not (os.path.exists(SHARED_SO) and all(os.path.getmtime(SHARED_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", SHARED_SO])
    lib = ctypes.CDLL(SHARED_SO)
    lib.sim_shared_open.restype = ctypes.c_void_p
    lib.sim_shared_digest.restype = ctypes.c_ulonglong
    lib.sim_shared_expire.restype = ctypes.c_longlong
    return lib


@pytest.fixture(scope="module")
def sim():
    lib = shared_lib()
    assert lib.sim_shared_row_bytes() == N.DECODED_DTYPE.itemsize and lib.sim_shared_sort_tile() == SORT_TILE
    return lib


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


class SimShared:
    """The shared decoder of n streams on the emulated kernels: the store and the host's bookkeeping live in the driver."""

    def __init__(self, lib, n_streams, filt, corr, fs, starts, slots=1 << 16, ages=False):
        self.lib = lib
        self.h = vp(lib.sim_shared_open(ctypes.c_int(n_streams), ctypes.c_longlong(slots), ctypes.c_int(corr == "Conservative"),
                                        ctypes.c_int(filt == "All Messages"), ctypes.c_int(ages), ctypes.c_double(fs)))
        for s, t in enumerate(starts):
            lib.sim_shared_set_start(self.h, ctypes.c_int(s), ctypes.c_double(t))

    def close(self):
        self.lib.sim_shared_close(self.h)

    def call(self, bits14, offset, stream, grid=3, dem=None, extra_items=(), rc=0):
        """One call's list: PDUs grouped by stream (a stream's PDUs contiguous), items in order of first appearance;
        extra_items: (position among the items, stream) of items without records.  -> (flags, rows, order, ts)"""
        b = np.ascontiguousarray(bits14, dtype=np.uint8)
        off = np.ascontiguousarray(offset, dtype=np.int64)
        stream = np.asarray(stream, dtype=np.int32)
        n = len(b)
        cut = np.concatenate([[0], np.flatnonzero(np.diff(stream)) + 1]).astype(np.int32) if n else np.zeros(0, np.int32)
        items = [(int(stream[c]), int(c)) for c in cut]
        for k, s in extra_items:
            items.insert(k, (s, items[k][1] if k < len(items) else n))
        assert len(set(s for s, _ in items)) == len(items), "a stream appears once per call"
        ist = np.array([s for s, _ in items], np.int32)
        first = np.array([f for _, f in items] + [n], np.int32)
        d = None if dem is None else np.ascontiguousarray(dem, dtype=np.uint8)
        flags, rows = np.zeros(n, np.uint16), np.zeros(n, dtype=N.DECODED_DTYPE)
        order, ts = np.zeros(n, np.int32), np.zeros(n, np.float64)
        got = self.lib.sim_shared_call(self.h, b.ctypes.data_as(vp), off.ctypes.data_as(vp), None if d is None else d.ctypes.data_as(vp),
                                       ctypes.c_int(n), ist.ctypes.data_as(vp), first.ctypes.data_as(vp), ctypes.c_int(len(items)),
                                       ctypes.c_int(grid), flags.ctypes.data_as(vp), rows.ctypes.data_as(vp), order.ctypes.data_as(vp),
                                       ts.ctypes.data_as(vp))
        assert got == rc, "guard overwritten (-1), bad key or order (-2), error word / books (-3), refused (-4), argument (-5): %d" % got
        return flags, rows, order, ts

    def reset(self):
        self.lib.sim_shared_reset(self.h)

    def set_max_cap(self, cap):
        self.lib.sim_shared_set_max_cap(self.h, ctypes.c_longlong(cap))

    def digest(self):
        return int(self.lib.sim_shared_digest(self.h))

    def stats(self):
        v = [ctypes.c_longlong() for _ in range(4)]
        self.lib.sim_shared_stats(self.h, *[ctypes.byref(x) for x in v])
        return dict(planes=v[0].value, capacity=v[1].value, grows=v[2].value, used=v[3].value)

    def planes(self):
        """{address: last_seen} read from the store"""
        cap = 1 << 16
        addr, seen = np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        n = self.lib.sim_shared_planes(self.h, addr.ctypes.data_as(vp), seen.ctypes.data_as(vp), ctypes.c_int(cap))
        assert n <= cap
        return dict(zip(addr[:n].tolist(), seen[:n].tolist()))

    def expire(self, cutoff, grid=3):
        r = int(self.lib.sim_shared_expire(self.h, ctypes.c_longlong(cutoff), ctypes.c_int(grid)))
        assert r >= 0, r
        return r


# ---- the golden ------------------------------------------------------------------------------------------------------------
def test_golden_holds_the_cases(g):
    """Cases (a) to (f) of tools/make_golden_shared.py, from the file alone."""
    ts, stream, call, order = g["ts"], g["stream"], g["call"], g["order"]
    n = len(ts)
    assert 250 <= n <= 600 and set(stream.tolist()) == {0, 1, 2, 3}
    assert np.array_equal(ts, g["start"][stream] + g["offset"].astype(np.float64) / float(g["fs"]))
    assert np.array_equal(order, np.concatenate([np.flatnonzero(call == c)[time_order(ts[call == c])] for c in range(call.max() + 1)]))
    for c in range(call.max() + 1):                   # a call's list: its items in the order passed, each one stream's records
        s = stream[call == c]
        heads = s[np.concatenate([[True], np.diff(s) != 0])].tolist()
        assert len(set(heads)) == len(heads) and [x for x in g["items_%d" % c].tolist() if x in heads] == heads
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    bits = np.unpackbits(g["bits"], axis=1)
    for tag in ("all_none", "all_cons"):
        has, icao, nm = g["has_" + tag], g["icao_" + tag], g["nmsgs_" + tag]
        # (a) even frames on stream 0 only, odd ones on stream 2 only, and a position in the end
        pa = 0x4B1A01
        pos = np.flatnonzero((icao == pa) & (g["df_" + tag] == 17) & (np.packbits(bits[:, 32:37], axis=1)[:, 0] >> 3 >= 9)
                             & (np.packbits(bits[:, 32:37], axis=1)[:, 0] >> 3 <= 18))
        assert len(pos) >= 4
        assert set(stream[pos[bits[pos, 53] == 0]].tolist()) == {0} and set(stream[pos[bits[pos, 53] == 1]].tolist()) == {2}
        k = g["f_icao_" + tag].tolist().index(pa)
        lat = g["f_lat_" + tag].view(np.float64)[k]
        assert not np.isnan(lat) and abs(lat - 47.11) < 0.02
        assert not np.isnan(g["lat_" + tag].view(np.float64)[pos[-1]])
        # (b) announced on stream 3 only, earlier in time and LATER in the list; the reply on stream 1 is known
        ann, rep = g["case_b"]
        assert stream[ann] == 3 and stream[rep] == 1 and call[ann] == call[rep] and ts[ann] < ts[rep] and ann > rep
        assert set(stream[(icao == icao[ann]) & (np.arange(n) != rep)].tolist()) == {3}
        assert has[rep] == 1 and icao[rep] == icao[ann] and nm[rep] == nm[ann] + 1
        # (c) announced later in time, EARLIER in the list: not known
        ann, rep = g["case_c"]
        assert call[ann] == call[rep] and ts[ann] > ts[rep] and ann < rep and has[rep] == 0 and has[ann] == 1 and nm[ann] == 1
        # (d) bit-equal timestamps, items passed as [1, 0, ...]: the reply's item first, so it is published first
        ann, rep = g["case_d"]
        assert ts[ann].tobytes() == ts[rep].tobytes() and stream[rep] == 1 and stream[ann] == 0 and rep < ann
        assert g["items_%d" % call[rep]].tolist()[:2] == [1, 0] and rank[rep] + 1 == rank[ann]
        assert has[rep] == 0 and has[ann] == 1 and nm[ann] == 1
        # (e) a call whose timestamps all precede the previous call's; its reply to an address of that call is known
        ann, rep = g["case_e"]
        assert call[rep] == call[ann] + 1 and ts[call == call[rep]].max() < ts[call == call[ann]].min()
        assert has[rep] == 1 and nm[rep] == nm[ann] + 1 and rank[rep] > rank[ann]
    # (f) a negative start beside positive ones, in one call
    assert g["start"][3] < 0 and (g["start"][:3] > 0).all()
    assert any((ts[call == c] < 0).any() and (ts[call == c] > 0).any() for c in range(call.max() + 1))
    # an empty item, so that items share a first record
    assert any(len(g["items_%d" % c]) > len(set(stream[call == c].tolist())) for c in range(call.max() + 1))


@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_replay_equals_golden(g, tag, filt, corr):
    rep = Replay(filt, corr)
    rows = np.zeros(len(g["ts"]), dtype=N.DECODED_DTYPE)
    for idx, _ in golden_calls(g, 0):
        rows[idx] = rows_of(rep.call(g["bits"][idx], g["ts"][idx])[1])
    TD.check_rows(rows, g, tag)
    planes = {a: t for a, t in zip(g["f_icao_" + tag].tolist(), g["f_seen_" + tag].tolist()) if a >= 0}
    assert rep.seen == planes


@pytest.mark.parametrize("partition", [0, 1])
@pytest.mark.parametrize("tag,filt,corr", CONFIGS)
def test_emulated_kernels_equal_golden(sim, g, tag, filt, corr, partition):
    """The golden's calls (and each cut in two by time) through the emulated kernels: order[], the records' verdict flags and
    the rows, against the reference's and byte for byte against the replays'."""
    f = SimShared(sim, 4, filt, corr, float(g["fs"]), g["start"].tolist(), slots=0, ages=True)
    rep = Replay(filt, corr)
    n = len(g["ts"])
    rows, flags = np.zeros(n, dtype=N.DECODED_DTYPE), np.zeros(n, np.uint16)
    pub = []
    for k, (idx, extra) in enumerate(golden_calls(g, partition)):
        fl, r, order, ts = f.call(g["bits"][idx], g["offset"][idx], g["stream"][idx], grid=1 + k % 3, extra_items=extra)
        assert ts.tobytes() == g["ts"][idx].tobytes()
        efl, er, eorder = rep.call(g["bits"][idx], g["ts"][idx])
        assert np.array_equal(order, eorder)
        assert np.array_equal(fl & AP_BITS, efl)
        S.assert_rows_equal(r, rows_of(er))
        rows[idx], flags[idx] = r, fl
        pub.append(idx[order])
    assert np.array_equal(np.concatenate(pub), g["order"])
    TD.check_rows(rows, g, tag)
    for case, known in (("case_b", True), ("case_c", False), ("case_d", False), ("case_e", True)):
        assert bool(flags[g[case][1]] & N.BURST_AP_KNOWN) == known, case
    planes = {a: t for a, t in zip(g["f_icao_" + tag].tolist(), g["f_seen_" + tag].tolist()) if a >= 0}
    assert f.planes() == planes and f.stats()["planes"] == len(planes)
    f.close()


# ---- the sort alone --------------------------------------------------------------------------------------------------------
def sort_ts(sim, ts, vals=None):
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    n = len(ts)
    order, keys = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    v = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
    assert sim.sim_shared_sort(ts.ctypes.data_as(vp), None if v is None else v.ctypes.data_as(vp), ctypes.c_int(n), order.ctypes.data_as(vp),
                               keys.ctypes.data_as(vp)) == 0, "a guard byte behind a sort buffer was overwritten"
    return order, keys


def sort_keys(sim, keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    order = np.zeros(len(keys), np.uint32)
    assert sim.sim_shared_sort_keys(keys.ctypes.data_as(vp), ctypes.c_int(len(keys)), order.ctypes.data_as(vp)) == 0
    return order


SORT_SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 3 * SORT_TILE + 1]


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_sizes(sim, n):
    """Random timestamps of both signs with many ties, at sizes around a wavefront and a tile: the order is sorted()'s."""
    rng = np.random.default_rng(n)
    ts = np.round(rng.normal(0, 50, n), 1) * rng.choice([1.0, 1e-300, 1e300, 1760000000.0], n)
    order, keys = sort_ts(sim, ts)
    assert np.array_equal(order, time_order(ts))
    assert np.all(keys[:-1] <= keys[1:])


@pytest.mark.parametrize("n", [65, 4097, 3 * SORT_TILE + 1])
def test_sort_is_stable(sim, n):
    """All keys equal: the identity.  Keys that differ in the top byte only, and in the bottom byte only: a stable sort by it."""
    assert np.array_equal(sort_ts(sim, np.full(n, 1760000000.25))[0], np.arange(n))
    rng = np.random.default_rng(n + 1)
    for shift in (56, 0):
        d = rng.integers(0, 256, n).astype(np.uint64)
        keys = np.uint64(0x00123456789ABC00 if shift == 56 else 0xFEDCBA9876543200) + (d << np.uint64(shift))
        assert np.array_equal(sort_keys(sim, keys), np.argsort(d, kind="stable"))
    # every digit of every pass in use, and values that are not 0 .. n-1 carried along
    keys = rng.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)
    assert np.array_equal(sort_keys(sim, keys), np.argsort(keys, kind="stable"))
    vals = rng.integers(0, 1 << 32, n).astype(np.uint32)
    ts = rng.integers(-3, 4, n).astype(np.float64)
    assert np.array_equal(sort_ts(sim, ts, vals)[0], vals[time_order(ts)])


def test_sort_signs_and_zeros(sim):
    """Negative and positive doubles mixed, denormals, infinities, and +-0.0, which compare equal: list order decides."""
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, np.inf, -np.inf, 1760000000.25, -1760000000.25, -0.0, 0.0, 2.0 ** -1022,
                        -2.0 ** -1022, 1.7976931348623157e308, -1.7976931348623157e308])
    rng = np.random.default_rng(5)
    ts = np.concatenate([special, rng.choice(special, 5000), -rng.random(300), rng.random(300)])
    order, _ = sort_ts(sim, ts)
    assert np.array_equal(order, time_order(ts))
    z = np.array([-0.0, 0.0, -0.0, 0.0, -1.0])
    assert sort_ts(sim, z)[0].tolist() == [4, 0, 1, 2, 3]


# ---- the host's rules, restated in the driver ------------------------------------------------------------------------------
FLEET = [0, 0xFFFFFF] + [0x500000 + 4099 * k for k in range(148)]
FS = 2e6
STARTS = [1760000100.25, 1760000100.75, 1760000099.5, -40.0]
_big = {}


def big_traffic():
    """Four streams of the same 150 aircraft: (bits, offset, stream, ts) per stream, about 600 PDUs each."""
    if "t" not in _big:
        out = []
        for s in range(4):
            b, t = S.mixed(np.random.default_rng(300 + s), n=600, addresses=FLEET, t0=0.0, dt=(0.002, 0.05))
            off = np.round(t * FS).astype(np.int64)
            out.append((b, off, np.full(len(b), s, np.int32), STARTS[s] + off.astype(np.float64) / FS))
        _big["t"] = out
    return _big["t"]


def big_calls(rng, lo=60, hi=200, first=None):
    """Calls of lo .. hi PDUs per stream (first: the first call's bounds), the streams in a random order, a random subset of them."""
    tr = big_traffic()
    at = [0] * 4
    if first is not None:
        (lo, hi), later = first, (lo, hi)
    while any(at[s] < len(tr[s][0]) for s in range(4)):
        live = [s for s in range(4) if at[s] < len(tr[s][0])]
        pick = [s for s in rng.permutation(live) if rng.random() < 0.8] or live[:1]
        parts = []
        for s in pick:
            k = int(rng.integers(lo, hi + 1))
            parts.append([x[at[s]:at[s] + k] for x in tr[s]])
            at[s] += k
        if first is not None:
            (lo, hi), first = later, None
        yield [np.concatenate([p[i] for p in parts]) for i in range(4)]


def test_store_grows_from_its_minimum_without_changing_a_row(sim):
    """About 150 aircraft heard by four receivers into a store at its minimum of 256 slots: growths, rows unchanged, one plane
    per aircraft whoever heard it."""
    for filt, corr in (("All Messages", "None"), ("All Messages", "Conservative")):
        f = SimShared(sim, 4, filt, corr, FS, STARTS, slots=0)
        rep = Replay(filt, corr)
        assert f.stats()["capacity"] == MIN_CAP
        for b, off, s, ts in big_calls(np.random.default_rng(11)):
            fl, r, order, _ = f.call(b, off, s)
            efl, er, eorder = rep.call(b, ts)
            assert np.array_equal(order, eorder) and np.array_equal(fl & AP_BITS, efl)
            S.assert_rows_equal(r, rows_of(er))
            st = f.stats()
            assert st["planes"] == len(rep.dec.planes) and 2 * st["used"] <= st["capacity"]
        assert st["grows"] >= 2 and 140 <= st["planes"] <= len(FLEET)
        f.close()


def test_a_refused_call_changes_nothing(sim):
    """A call the store has no room for is refused before any kernel touches the store: the state's digest stays, and the
    call, repeated with room, gives the rows of a run that was never refused."""
    calls = list(big_calls(np.random.default_rng(12), first=(10, 20)))[:4]          # the first fits the 256 slots, the second does not
    clean = SimShared(sim, 4, "All Messages", "None", FS, STARTS, slots=0)
    want = [clean.call(b, off, s) for b, off, s, _ in calls]
    f = SimShared(sim, 4, "All Messages", "None", FS, STARTS, slots=0)
    got = [f.call(*calls[0][:3])]
    f.set_max_cap(f.stats()["capacity"])
    before = f.digest()
    b, off, s, _ = calls[1]
    assert 2 * (f.stats()["used"] + len(b)) > f.stats()["capacity"]
    f.call(b, off, s, rc=-4)
    assert f.digest() == before
    f.set_max_cap(1 << 27)
    got += [f.call(b, off, s) for b, off, s, _ in calls[1:]]
    for (gfl, gr, go, _), (wfl, wr, wo, _) in zip(got, want):
        assert np.array_equal(gfl, wfl) and np.array_equal(go, wo) and gr.tobytes() == wr.tobytes()
    assert f.digest() == clean.digest()
    f.close(), clean.close()


def test_decoder_reset_is_a_stream_reset_of_the_one_decoder(sim):
    """adsb_streams_decoder_reset against adsb_stream_reset: one stream with whole-second timestamps through the per-stream
    driver and its reset, and through the shared driver and its reset -- the same rows before and after, a fresh decoder's."""
    import test_stream_decode as TS
    fleet = TS.SimFleet(TS.fleet_lib(), 1, "All Messages", "None", slots=0)
    b, t = S.mixed(np.random.default_rng(13), n=400, addresses=FLEET[:40], t0=1760000000.0, dt=(0.2, 1.5))
    t = np.floor(t)
    f = SimShared(sim, 1, "All Messages", "None", 1.0, [0.0], slots=0)
    off, s = t.astype(np.int64), np.zeros(len(b), np.int32)
    first = f.call(b[:250], off[:250], s[:250])[1]
    assert first.tobytes() == fleet.call(b[:250], t[:250], s[:250]).tobytes()
    assert f.stats()["planes"] == 40
    f.reset(), fleet.reset(0)
    assert f.stats()["planes"] == 0 and f.planes() == {}
    again = f.call(b[250:], off[250:], s[250:])[1]
    assert again.tobytes() == fleet.call(b[250:], t[250:], s[250:]).tobytes()
    S.assert_rows_equal(again, D.Decoder("All Messages", "None").rows(b[250:], t[250:]))
    f.close(), fleet.close()


def test_records_without_a_pdu_take_part_in_the_order_and_publish_nothing(sim):
    b, off, s, ts = next(big_calls(np.random.default_rng(14)))
    dem = np.random.default_rng(15).random(len(b)) < 0.7
    f = SimShared(sim, 4, "All Messages", "None", FS, STARTS)
    rep = Replay("All Messages", "None")
    fl, r, order, _ = f.call(b, off, s, dem=dem)
    efl, er, eorder = rep.call(b, ts, dem=dem)
    assert np.array_equal(order, eorder) and np.array_equal(fl & AP_BITS, efl)
    S.assert_rows_equal(r[dem], rows_of(er))
    assert not (r["port"][~dem]).any() and not (r["present"][~dem]).any() and not (fl[~dem] & N.BURST_DEMOD).any()
    f.close()


def test_plane_ages_and_expiry(sim):
    """ADSB_FLAG_PLANE_AGES: after every call the decoder's last_seen clocks are the replay's; expiring the older half leaves
    later rows those of the replay with those keys deleted."""
    f = SimShared(sim, 4, "All Messages", "None", FS, STARTS, slots=0, ages=True)
    rep = Replay("All Messages", "None")
    calls = list(big_calls(np.random.default_rng(16)))
    for k, (b, off, s, ts) in enumerate(calls):
        r = f.call(b, off, s)[1]
        S.assert_rows_equal(r, rows_of(rep.call(b, ts)[1]))
        assert f.planes() == rep.seen
        if k == len(calls) // 2:
            cutoff = int(np.median([v for v in rep.seen.values() if v > 0]))
            n = rep.expire(cutoff)
            assert 10 <= n < len(rep.seen) + n and f.expire(cutoff) == n
            assert f.planes() == rep.seen and f.stats()["planes"] == len(rep.seen)
    f.close()


# ---- build facts -----------------------------------------------------------------------------------------------------------
def test_kernel_resources_shared():
    """The new translation unit's report: the k_shared_* kernels, none with scratch or spills; the scatter's LDS is the
    documented 5 KiB."""
    from gr_adsb_amd import build as B
    B.build()
    res = json.load(open(B.RES_SHARED))
    names = sorted(re.search(r"k_shared_[a-z_]+?(?=E)", k).group(0) for k in res)
    assert names == ["k_shared_gather", "k_shared_keys", "k_shared_scatter", "k_shared_sort_hist", "k_shared_sort_scan",
                     "k_shared_sort_scatter"], sorted(res)
    for k, v in res.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    lds = {re.search(r"k_shared_[a-z_]+?(?=E)", k).group(0): v["lds_bytes_per_block"] for k, v in res.items()}
    assert lds["k_shared_sort_scatter"] == 5 * 1024 and lds["k_shared_sort_hist"] == 1024
    assert lds["k_shared_keys"] == lds["k_shared_gather"] == lds["k_shared_scatter"] == 0
    assert not any("k_shared" in k for k in json.load(open(B.RES)))


def test_side_copies_are_built_from_both_units():
    """tools/kbench.py builds its side copies of the library through build.compile_and_link, which compiles both translation
    units with build.FLAGS -- the flags of a shared library, as before the second unit."""
    from gr_adsb_amd import build as B
    assert "-shared" in B.FLAGS and "-c" not in B.FLAGS and B.SOURCES == ["adsb_hip.hip"] and B.SHARED_SOURCE == "adsb_shared.hip"
    src = open(os.path.join(HERE, "..", "tools", "kbench.py")).read()
    assert "b.compile_and_link(out, flags.split()" in src and "b.FLAGS" not in src


def test_flag_and_abi_constants():
    hdr = open(os.path.join(HERE, "..", "include", "adsb_hip.h")).read()
    assert re.search(r"#define ADSB_FLAG_STREAM_DECODE_SHARED (\d+)u", hdr).group(1) == str(N.FLAG_STREAM_DECODE_SHARED) == "4096"
    assert re.search(r"#define ADSB_ABI_VERSION (\d+)", hdr).group(1) == "5" and N.ABI_VERSION == 5
    for name in ("adsb_stream_last_order", "adsb_streams_decoder_reset"):
        assert name in N.EXPORTS and re.search(r"^int %s\(" % name, hdr, re.M)
