"""noise_median (adsb_device.h) by itself, on the SIMT emulator: every window of tests/median_cases.py through both instances,
against median_cases.median_ref, with the turns it took (ADSB_MEDIAN_PATH) against the ones each case was built for and against
median_cases.predict.  tests/test_gpu_units.py runs the same arrays on the MI355X.

The reference itself is held to np.median, as bits, on every generated window.  One exception is written into the issue's own
list of fixed NaN bits: np.median hands back the NaN it found (sign and payload of the sample), the device -- like the C oracle's
sum -- the canonical 0x7FC00000; for a window that holds a NaN the check is that np.median is a NaN too."""
import warnings

import numpy as np
import pytest

import median_cases as M
import simlib

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def units():
    return simlib.Units(simlib.lib())


@pytest.fixture(scope="module", params=[False, True], ids=["float", "quant"])
def run(request, units):
    """(quant, chains, (windows, nwin, start, hint0), (median, key, hint seen), emulator's (median, hint, path))"""
    quant = request.param
    chains, packed, ref = M.all_chains(quant)
    return quant, chains, packed, ref, units.noise_median(quant, *packed)


def names(word):
    return {n for k, n in enumerate(M.PATHS) if (int(word) >> k) & 1}


def test_path_names_match_the_header():
    assert simlib.lib().sim_median_path_count() == len(M.PATHS) == len(simlib.MEDIAN_PATHS)
    assert tuple(M.PATHS) == tuple(simlib.MEDIAN_PATHS)


def test_key_map_is_monotone_and_inverts():
    rng = np.random.default_rng(7)
    v = np.concatenate([M.f32(rng.integers(0, 1 << 32, 4096)), np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32)])
    v = v[~np.isnan(v)]
    k = M.key_of(v)
    assert np.array_equal(M.bits_of(M.unkey(k)), M.bits_of(v))
    order = np.argsort(k, kind="stable")
    assert np.all(np.diff(v[order].astype(np.float64)) >= 0)
    assert M.key_of(np.float32(-0.0)) + 1 == M.key_of(np.float32(0.0)) and int(M.key_of(np.float32(1.0))) == M.K_ONE


def test_reference_equals_numpy_median_on_every_window():
    seen = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for quant in (False, True):
            chains = M.all_chains(quant)[0]
            for ch in chains if not quant else [c for c in chains if c.name.startswith("random_")]:
                for w in ch.windows:
                    got = M.median_ref(w)[0]
                    want = np.float32(np.median(w))
                    if np.isnan(w).any():
                        assert np.isnan(want) and got == M.NAN_WINDOW, ch.name
                    else:
                        assert got == int(want.view(np.uint32)), (ch.name, len(w), hex(got), hex(int(want.view(np.uint32))))
                    seen += 1
    assert seen > 2 * 4096
    assert M.median_ref(np.array([-np.inf, np.inf], dtype=np.float32))[0] == 0xFFC00000
    assert M.median_ref(np.zeros(0, dtype=np.float32)) == (0xFFC00000, 0)
    assert M.median_ref(np.array([-0.0, -0.0], dtype=np.float32))[0] == 0
    assert M.median_ref(M.f32([1, 2]))[0] == 2 and M.median_ref(M.f32([3, 4]))[0] == 4          # halves round to even


def test_generators_repeat():
    a, b = M.pack(M.named_chains() + M.random_chains(True, 64)), M.pack(M.named_chains() + M.random_chains(True, 64))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    chains = M.named_chains()
    assert {len(w) for c in chains for w in c.windows} >= set(M.LENGTHS)
    assert len({c.name for c in chains}) == len(chains)


def test_median_bits_and_hint_equal_the_reference(run):
    quant, chains, (windows, nwin, start, hint0), (med, key, _), (got_med, got_hint, _) = run
    assert len(got_med) == len(med) == start[-1] and len(chains) == len(start) - 1
    bad = np.flatnonzero(got_med != med)
    which = [(chains[np.searchsorted(start, b, side="right") - 1].name, int(nwin[b]), hex(got_med[b]), hex(med[b])) for b in bad[:5]]
    assert len(bad) == 0, (len(bad), which)
    bad = np.flatnonzero(got_hint != key)
    which = [(chains[np.searchsorted(start, b, side="right") - 1].name, int(nwin[b]), hex(got_hint[b]), hex(key[b])) for b in bad[:5]]
    assert len(bad) == 0, (len(bad), which)
    assert np.all(got_hint[nwin == 0] == 0)


def test_named_cases_take_the_path_they_were_built_for(run):
    quant, chains, (_, _, start, _), _, (_, _, path) = run
    checked = 0
    for c, ch in enumerate(chains):
        for k in range(len(ch.windows)):
            want = ch.expected(k, quant)
            if want:
                got = names(path[start[c] + k])
                assert want <= got, (ch.name, k, sorted(want), sorted(got))
                checked += 1
    assert checked > 600


def test_every_window_takes_the_predicted_path(run):
    """no window is skipped: one hint outcome each, one exit unless the hint was exact, one upper-middle outcome unless the
    window is empty or holds a NaN -- and they are the ones the contract names"""
    quant, chains, (_, _, start, _), (_, _, hint_seen), (_, _, path) = run
    for c, ch in enumerate(chains):
        for k, w in enumerate(ch.windows):
            i = start[c] + k
            got, want = names(path[i]), M.predict(w, int(hint_seen[i]), quant)
            assert got == want, (ch.name, k, len(w), hex(int(hint_seen[i])), sorted(got), sorted(want))
            assert len(got & set(M.HINTS)) == 1 and len(got & set(M.EXITS)) == (0 if "hint_exact" in got else 1)
            assert len(got & set(M.UPPERS)) == (0 if len(w) == 0 or np.isnan(w).any() else 1)


def test_every_path_occurs(run):
    quant, _, _, _, (_, _, path) = run
    count = {n: int(np.count_nonzero((path >> k) & 1)) for k, n in enumerate(M.PATHS)}
    print(("quant" if quant else "float"), count)
    for n in M.PATHS:
        if n in ("hint_exact", "upper_exact_again"):
            assert (count[n] > 0) == quant, (n, count[n])     # the exact hit exists in the QUANT instance only
        else:
            assert count[n] > 0, n
