"""The time order's kernels on the MI355X itself, at the seams tests/test_shared_decode.py puts the pair sort to on the SIMT
emulator: the shipped translation unit gr_adsb_amd/csrc/adsb_shared.hip, compiled with the library's flags, and its real
launchers with their own cover() and blocks(), driven by tests/gpu/shared_device_driver.hip -- every array a part of its own in
device memory with a guard tail, every part read back whole behind every launcher.

(a) test_shared_decode.py's test_sort_sizes, test_sort_is_stable and test_sort_signs_and_zeros, imported unchanged, with this
    module's `sim`: what hipcc made of k_shared_sort_scatter's ballots and k_shared_sort_scan's __shfl_up scan.
(b) The chain launch_keys -> launch_sort -> launch_gather -> launch_scatter at n = 1, 255, 256, 257 and 4097: offsets of both
    signs up to +-2^62, a negative start, empty first, middle and last items, timestamps that tie.  ts bit-equal to
    start[item] + offset.astype(float64) / fs, keys to shared_replay.time_key_np of those bits, order to
    shared_replay.time_order, gather and scatter to fancy indexing; all words distinct, so a word in the wrong place shows.
(c) The chain at n = 58 255, where k_shared_scatter alone goes round its grid-stride loop again, and at n = 2048 * 256 + 257,
    where k_shared_keys and k_shared_gather do too and the sort has 129 blocks: k_shared_sort_scan runs 129 rounds with its carry.
Every output is an integer or a bit pattern: no tolerance, no comparison with the emulator's bytes."""
import ctypes

import numpy as np
import pytest

import device_build
from shared_replay import time_key_np, time_order
from test_shared_decode import SORT_TILE, test_sort_is_stable, test_sort_signs_and_zeros, test_sort_sizes      # noqa: F401

pytestmark = pytest.mark.gpu

COVER_CAP = 2048 * 256            # threads of the largest grid cover() gives
FS = 2e6
vp = ctypes.c_void_p
ran = {"imported": 0, "calls": 0}


class Device:
    """the device library's entries; after every call the library must still be alive"""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*a):
            rc = fn(*a)
            ran["calls"] += 1
            assert self.lib.dev_shared_dead() == 0, "a HIP call failed (%d): no further GPU call is made" % rc
            return rc
        return call


@pytest.fixture(scope="module")
def sim():
    import torch                  # first, as _native.load() does: the library must bind to the HIP runtime torch bundles, or the
    assert torch.cuda.is_available(), "GPU tests need a GPU"      # process holds two runtimes and the later one finds no device
    so = device_build.device_lib("adsb_shared.hip", "shared_device_driver.hip", "libadsb_shared_dev.so", ("adsb_shared.h", "adsb_shared_device.h"))
    dev = Device(ctypes.CDLL(so))
    assert dev.sim_shared_sort_tile() == SORT_TILE
    return dev


@pytest.fixture(autouse=True)
def count_imported(request):
    yield
    ran["imported"] += request.function.__module__ == "test_shared_decode"


def distinct_words(rng, shape, base):
    """random 64-bit words that differ pairwise, from one another and from every other call's with another `base`: 40 random
    bits over a running number of 24"""
    k = int(np.prod(shape))
    assert base + k <= 1 << 24
    return ((rng.integers(0, 1 << 40, k).astype(np.uint64) << np.uint64(24)) | (base + np.arange(k)).astype(np.uint64)).reshape(shape)


def chain_world(n, seed):
    """-> the chain's arguments: six items -- an empty first, an empty middle and an empty last one among three with records
    (n = 1: one) --, starts of both signs, offsets that tie, realistic ones and ones of both signs up to +-2^62"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, 2))
    first = np.array([0, 0, cuts[0], cuts[0], cuts[1], n, n], np.int32)
    start = np.array([5.0, 1760000100.25, -3.5, -40.0, 1760000099.5, 7.0])
    kind = rng.integers(0, 4, n)
    off = np.where(kind == 0, rng.integers(0, 64, n),                                 # few values: timestamps tie within an item
                   np.where(kind == 1, rng.integers(0, 1 << 31, n),
                            np.where(kind == 2, -rng.integers(0, 1 << 31, n), rng.integers(-(1 << 62), (1 << 62) + 1, n)))).astype(np.int64)
    if n >= 4:
        off[:4] = [1 << 62, -(1 << 62), (1 << 62) - 1, -(1 << 53) - 1]
    recs = distinct_words(rng, (n, 4), 0)
    recs[:, 0] = off.view(np.uint64)                                   # word 0 is the offset: the one word that repeats, where timestamps tie
    rows = distinct_words(rng, (n, 9), 4 * n)
    delivered = distinct_words(rng, (n, 4), 13 * n)
    return first, start, off, recs, rows, delivered


def run_chain(sim, n, seed):
    first, start, off, recs, rows, delivered = chain_world(n, seed)
    item = np.repeat(np.arange(len(start)), np.diff(first))
    assert len(item) == n and first[0] == first[1] and first[-1] == first[-2] and first[2] == first[3] and (start < 0).any()
    out = dict(ts=np.zeros(n, np.float64), keys=np.zeros(n, np.uint64), order=np.zeros(n, np.int32), srecs=np.zeros((n, 4), np.uint64),
               sts=np.zeros(n, np.float64), recs=np.zeros((n, 4), np.uint64), rows=np.zeros((n, 9), np.uint64))
    rc = sim.dev_shared_chain(recs.ctypes.data_as(vp), ctypes.c_int(n), first.ctypes.data_as(vp), start.ctypes.data_as(vp),
                              ctypes.c_int(len(start)), ctypes.c_double(FS), rows.ctypes.data_as(vp), delivered.ctypes.data_as(vp),
                              *[out[k].ctypes.data_as(vp) for k in ("ts", "keys", "order", "srecs", "sts", "recs", "rows")])
    assert rc == 0, "guard or read-only input (-1), no permutation (-2), argument (-5), a HIP status (<= -1000): %d" % rc
    ts = start[item] + off.astype(np.float64) / FS
    assert out["ts"].tobytes() == ts.tobytes(), ("ts", n, np.flatnonzero(out["ts"].view(np.uint64) != ts.view(np.uint64))[:5])
    assert out["keys"].tobytes() == time_key_np(ts).tobytes(), ("keys", n)
    order = time_order(ts.tolist()).astype(np.int32)
    assert (np.diff(ts[order]) == 0).any() or n < 255, "timestamps tie: the list position decides"
    assert out["order"].tobytes() == order.tobytes(), ("order", n, np.flatnonzero(out["order"] != order)[:5])
    assert out["srecs"].tobytes() == recs[order].tobytes() and out["sts"].tobytes() == ts[order].tobytes(), ("gather", n)
    want_rows = np.zeros_like(rows)
    want_rows[order] = rows
    want_recs = delivered.copy()
    want_recs[order, 3] = recs[order, 3]
    assert out["rows"].tobytes() == want_rows.tobytes(), ("scatter: rows", n, np.flatnonzero((out["rows"] != want_rows).any(1))[:5])
    assert out["recs"][:, :3].tobytes() == delivered[:, :3].tobytes(), ("scatter: words 0 to 2 of the delivered records", n)
    assert out["recs"].tobytes() == want_recs.tobytes() and not (delivered[:, 3] == recs[:, 3]).any(), ("scatter: word 3", n)


@pytest.mark.parametrize("n", [1, 255, 256, 257, SORT_TILE + 1])
def test_the_chain(sim, n):
    """(b): around a workgroup of the grid-stride kernels, and one sort tile and one"""
    run_chain(sim, n, n)


N_SCATTER = 58255                 # * 9 row words: the first size at which k_shared_scatter's work exceeds the largest grid
N_ALL = COVER_CAP + 257


def test_the_second_grid_stride_round(sim):
    """(c): from the sizes alone, at N_SCATTER only k_shared_scatter's work exceeds the largest grid, at N_ALL k_shared_keys'
    and k_shared_gather's do too, and the sort has 129 blocks -- 129 rounds of k_shared_sort_scan with its carry."""
    assert (N_SCATTER - 1) * 9 <= COVER_CAP < N_SCATTER * 9 and N_SCATTER <= COVER_CAP
    assert N_ALL > COVER_CAP and -(-N_ALL // SORT_TILE) == 129 and 129 * 256 // 256 == 129
    for n in (N_SCATTER, N_ALL):
        run_chain(sim, n, n)
        print("stride: the chain at %d records, %d row words, %d sort blocks" % (n, n * 9, -(-n // SORT_TILE)))


def test_the_imported_cases_ran():
    """runs last in this file: says how many of test_shared_decode.py's cases ran on the device"""
    print("device: %d imported cases, %d calls of the device library" % (ran["imported"], ran["calls"]))
    assert ran["calls"] > ran["imported"] > 0
