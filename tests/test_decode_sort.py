"""ADSB_FLAG_DECODE's group stage alone on the CPU: k_dec_sort_hist / k_dec_sort_scan / k_dec_sort_scatter on the SIMT
emulator, in launch_dec's order (tests/sim/decode_driver.cpp sim_dec_sort), against NumPy's stable argsort of bits 32..59.
Equality element for element: a permutation, ordered by address, list order inside an address, kDecNoKey last.

Sizes around every boundary of the kernels: a wave (64), a round (256 threads), a tile (4096 keys per workgroup), two tiles,
16 tiles (the scan sees exactly 256 entries, one round) and 16 tiles + 1 key (17 workgroups: the scan's carry), and a few
tiles plus a remainder.  The emulator costs as much per started tile as per full one, so the random mix -- every digit value
in every workgroup, the lowest and the highest address, keys without an address -- runs at every size, the other patterns at
one size of each kind, and those that fill the scan's second round (the highest address, keys without one) at 16 tiles + 1."""
import ctypes

import numpy as np
import pytest

from test_decode import dec_lib

NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)
TILE = 4096
SIZES = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 3 * TILE + 777, 65536, 65537)
SOME = (17, 257, 4097, 8193)            # below a wave, a round + 1, a tile + 1, two tiles + 1


@pytest.fixture(scope="module")
def sim():
    lib = dec_lib()
    assert lib.sim_dec_sort_tile() == TILE
    return lib


def keys_of(addr, nokey=None):
    """address << 32 | position, as k_dec_classify writes them; kDecNoKey where nokey is set."""
    addr = np.asarray(addr, dtype=np.uint64)
    k = (addr << np.uint64(32)) | np.arange(len(addr), dtype=np.uint64)
    if nokey is not None:
        k[nokey] = NOKEY
    return k


def check_sort(lib, k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    out = np.full(len(k), np.uint64(0x1111111111111111), dtype=np.uint64)
    vp = ctypes.c_void_p
    rc = lib.sim_dec_sort(k.ctypes.data_as(vp), ctypes.c_int(len(k)), out.ctypes.data_as(vp))
    assert rc == 0, "a sort kernel wrote outside its %d keys" % len(k)
    exp = k[np.argsort((k >> np.uint64(32)) & np.uint64(0xFFFFFFF), kind="stable")]
    bad = np.flatnonzero(out != exp)
    assert len(bad) == 0, (len(k), len(bad), bad[:5], [hex(int(x)) for x in out[bad[:3]]], [hex(int(x)) for x in exp[bad[:3]]])


def random_mix(rng, n):
    """Addresses of every digit in every tile: a few busy aircraft, many rare ones, 0 and 0xFFFFFF, a fifth without a key."""
    busy = np.concatenate([[0, 0xFFFFFF, 0xFFFFF0, 0x0FFFFF], rng.integers(0, 1 << 24, 12)])
    addr = np.where(rng.random(n) < 0.5, rng.choice(busy, n), rng.integers(0, 1 << 24, n))
    return keys_of(addr, rng.random(n) < 0.2)


@pytest.mark.parametrize("n", SIZES)
def test_random_mix(sim, n):
    check_sort(sim, random_mix(np.random.default_rng(n), n))


@pytest.mark.parametrize("n", SOME)
def test_one_address_throughout(sim, n):
    check_sort(sim, keys_of(np.full(n, 0x4B1A2C)))


@pytest.mark.parametrize("n", SOME + (65537,))
def test_distinct_descending_addresses(sim, n):
    check_sort(sim, keys_of(0xFFFFFF - 251 * np.arange(n)))


@pytest.mark.parametrize("n", SOME + (65536, 65537))
def test_only_the_lowest_and_the_highest_address(sim, n):
    rng = np.random.default_rng(n + 1)
    check_sort(sim, keys_of(np.where(rng.random(n) < 0.5, 0, 0xFFFFFF)))


@pytest.mark.parametrize("n", SOME)
def test_every_key_is_no_key(sim, n):
    check_sort(sim, np.full(n, NOKEY))


@pytest.mark.parametrize("n", SOME)
@pytest.mark.parametrize("k", (2, 5, 65))
def test_no_key_interleaved_one_in_k(sim, n, k):
    rng = np.random.default_rng(n + k)
    check_sort(sim, keys_of(rng.integers(0, 1 << 24, n), np.arange(n) % k == k - 1))


@pytest.mark.parametrize("n", (257, 2 * TILE + 1))
@pytest.mark.parametrize("digit", range(6))
def test_addresses_that_differ_in_one_digit(sim, n, digit):
    """Only one of the seven passes moves anything; the others must keep the order they were given."""
    rng = np.random.default_rng(n + digit)
    check_sort(sim, keys_of(0xA5A5A5 & ~(0xF << (4 * digit)) | (rng.integers(0, 16, n) << (4 * digit))))


@pytest.mark.parametrize("n", (4097, 8193, 3 * TILE + 777))
def test_real_keys_only_in_the_last_tile(sim, n):
    rng = np.random.default_rng(n + 2)
    last = (n - 1) // TILE * TILE
    check_sort(sim, keys_of(rng.integers(0, 1 << 24, n), np.arange(n) < last))


@pytest.mark.parametrize("n", (4096, 8193, 3 * TILE + 777))
def test_real_keys_only_at_each_tiles_first_and_last_slot(sim, n):
    rng = np.random.default_rng(n + 3)
    pos = np.arange(n)
    edge = (pos % TILE == 0) | (pos % TILE == TILE - 1) | (pos == n - 1)
    check_sort(sim, keys_of(rng.choice([7, 0xFFFFFF, 0, 0x800000], n), ~edge))
