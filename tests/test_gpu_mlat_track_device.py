"""The MLAT track store's kernels on the MI355X itself, at the cases tests/test_mlat_track.py puts them to on the SIMT emulator: the
shipped translation unit gr_adsb_amd/csrc/adsb_mlat_track.hip, compiled with the library's flags, and its real launchers with
their own cover(), driven by tests/gpu/mlat_track_device_driver.hip -- the emulator driver's entry points on device memory, every
array a part of its own with a guard tail, every part read back whole behind every launch group (tests/sim/mlat_track_host_rule.h
is both drivers' host rule).

(a) test_mlat_track.py's cases, imported unchanged, with this module's `sim`: what hipcc made of the kernels against the replay,
    byte for byte.
(b) Every update, readout and expiry of (a) over at most TWIN_MAX fixes or rows is repeated on the emulator library with the
    same arguments; the stores, the rows, the stats, the counts and the return codes are compared as bytes, and
    test_the_device_equals_the_emulator_byte_for_byte, which runs last, asserts that none differed.
(c) test_the_second_grid_stride_round: 2048 * 256 + 300 runs -- one fix each of as many addresses -- so that k_track_find and
    k_track_update, one lane per run under cover()'s cap of 2048 workgroups of 256, go round their grid-stride loops a second
    time (and every kernel over the keys with them); then as many fixes again onto that store, which k_track_move strides over
    a dozen times.  The smallest such count but for the margin of 300."""
import ctypes

import numpy as np
import pytest

import device_build
import test_mlat_track as TT
from gr_adsb_amd import _native as N
from test_mlat_track import (test_no_fix_one_fix_and_no_eligible_fix, test_the_smallest_and_the_largest_address, test_unusable_fixes,      # noqa: F401
                             test_equal_timestamps_are_stale, test_the_gap, test_the_gate, test_restart_after,
                             test_a_track_begun_on_an_outlier_recovers, test_a_run_longer_than_a_chunk,
                             test_a_run_across_a_chunk_and_a_sort_tile_boundary, test_many_addresses_in_shuffled_rows, test_the_merge,
                             test_a_second_identical_call_changes_nothing, test_a_rejected_fix_is_not_remembered, test_the_rule_is_refused, test_expiry, test_the_readout,
                             test_the_sizing_rule, test_a_moving_aircraft)

pytestmark = pytest.mark.gpu

TWIN_MAX = 4096
COVER_CAP = 2048 * 256


class Both:
    """test_mlat_track.Lib of the device library; every call of at most TWIN_MAX fixes (or rows, for the readout and the expiry)
    is repeated on the emulator's, and what differs is kept for the module's last test"""

    def __init__(self, dev, emu):
        self.dev, self.emu, self.compared, self.differ = dev, emu, 0, []

    def alive(self):
        assert self.dev.lib.dev_track_dead() == 0, "a HIP call failed: no further GPU call is made"

    def twin(self, what, size, got, again):
        if size > TWIN_MAX:
            return
        exp = again()
        self.compared += 1
        same = len(got) == len(exp) and all((g.tobytes() == e.tobytes()) if isinstance(g, np.ndarray) else g == e for g, e in zip(got, exp))
        if not same:
            self.differ.append((what, size, got, exp))

    def update(self, fixes, aux, rule, store):
        got = self.dev.update(fixes, aux, rule, store)
        self.alive()
        self.twin("update", len(fixes), got, lambda: self.emu.update(fixes, aux, rule, store))
        return got

    def read(self, store, min_fixes=1, cutoff=-np.inf, cap=None):
        got = self.dev.read(store, min_fixes, cutoff, cap)
        self.alive()
        self.twin("read", len(store), got, lambda: self.emu.read(store, min_fixes, cutoff, cap))
        return got

    def expire(self, store, cutoff):
        got = self.dev.expire(store, cutoff)
        self.alive()
        self.twin("expire", len(store), (got,), lambda: (self.emu.expire(store, cutoff),))
        return got

    def layout(self, n):
        assert self.dev.layout(n) == self.emu.layout(n)
        return self.dev.layout(n)

    def cover(self, work, per):
        return self.dev.cover(work, per)

    def sort_tile(self):
        return self.dev.sort_tile()


@pytest.fixture(scope="module")
def sim():
    import torch                  # first, as _native.load() does: the library must bind to the HIP runtime torch bundles
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    so = device_build.device_lib("adsb_mlat_track.hip", "mlat_track_device_driver.hip", "libadsb_mlat_track_dev.so",
                                 ("adsb_mlat_track.h", "adsb_mlat_track_device.h", "adsb_shared.hip", "adsb_shared.h", "adsb_shared_device.h"))
    return Both(TT.Lib(ctypes.CDLL(so)), TT.Lib(TT.track_lib()))


def test_the_second_grid_stride_round(sim):
    """(c): the rule's outcome for one fix per address and for a second fix of each is stated without the replay's loop: every
    first fix starts a track, every second one is taken with p = f0 + alpha d, v = (beta / dt) d."""
    n = COVER_CAP + 300
    assert sim.cover(n, 256) == 2048 and n > COVER_CAP
    rng = np.random.default_rng(11)
    icao = rng.permutation(1 << 24)[:n].astype(np.int32)
    p0 = TT.P0 + rng.normal(0, 1e5, (n, 3))
    f, a = TT.make_fixes(icao, 10.0 + np.arange(n) * 1e-6, p0)
    rule = N.mlat_track_rule()
    rc, store, stats = sim.update(f, a, rule, TT.EMPTY)
    assert rc == 0 and stats == dict(fixes=n, eligible=n, unusable=0, stale=0, rejected=0, taken=0, started=n, tracks=n)
    order = np.argsort(icao, kind="stable")
    assert np.array_equal(store["icao"], icao[order]) and (store["n_fixes"] == 1).all() and (store["flags"] == 0).all()
    for k, name in enumerate("xyz"):
        assert np.array_equal(store[name], p0[order, k]) and (store["v" + name] == 0.0).all()
    assert np.array_equal(store["last_ts"], f["ts"][order]) and np.array_equal(store["first_ts"], f["ts"][order])
    d = rng.normal(0, 200.0, (n, 3))
    f2, a2 = TT.make_fixes(icao, 12.0 + np.arange(n) * 1e-6, p0 + d, rms=33.0, n_rx=5)
    rc, store2, stats = sim.update(f2, a2, rule, store)
    assert rc == 0 and stats == dict(fixes=n, eligible=n, unusable=0, stale=0, rejected=0, taken=n, started=0, tracks=n)
    dt = f2["ts"] - f["ts"]
    for k, name in enumerate("xyz"):
        dd = (p0 + d)[:, k] - (p0[:, k] + 0.0 * dt)
        assert np.array_equal(store2[name], ((p0[:, k] + 0.0 * dt) + np.float64(0.3) * dd)[order])
        assert np.array_equal(store2["v" + name], (0.0 + (np.float64(0.05) / dt) * dd)[order])
    assert (store2["n_fixes"] == 2).all() and (store2["rms_m"] == 33.0).all() and (store2["n_rx"] == 5).all()
    assert np.array_equal(store2["icao"], store["icao"]) and np.array_equal(store2["last_ts"], f2["ts"][order])


def test_the_device_equals_the_emulator_byte_for_byte(sim):
    """(b), runs last in this file: of the calls above that both libraries took, none differed in a byte"""
    assert sim.compared > 20, "the cases above ran"
    print("device = emulator over %d calls" % sim.compared)
    assert not sim.differ, (len(sim.differ), [(w, s) for w, s, _, _ in sim.differ[:5]])
