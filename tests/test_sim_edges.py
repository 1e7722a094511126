"""The edge-case matrix of tests/edge_cases.py on the CPU SIMT emulator (the shipped adsb_device.h compiled for the host):
every input format -- int8 and uint8 at power-of-two scales reach the dot-product instances k_detect<5|6, .> through the
emulator's own dispatch (sim_driver.cpp, like the library's launch_detect) -- at 2 and 8 Msps and one run-time stride
(6 Msps), bit for bit against the C oracle on the oracle's |IQ|^2 of the same bytes."""
import warnings

import numpy as np
import pytest

import edge_cases as E
import simlib
from helpers import assert_recs_equal
from oracle import c_oracle as C

RATES = (2e6, 8e6, 6e6)


def test_generator_geometry_is_the_kernels():
    tile, fwd, _ = simlib.kernel_geometry()
    assert (E.TILE, E.FWD) == (tile, fwd)


def _run(fmt, scale, fs, full):
    mode = E.FORMATS[fmt][0]
    sps = int(fs // 1e6)
    n_cases = n_recs = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, data, x, thr in E.cases(fmt, scale, sps, full=full):
            want = C.canonical(x, sps, thr)
            got, so = simlib.sim_canonical(mode, data, fs, thr, scale=1.0 if scale is None else scale)
            assert so.overflow == 0
            assert_recs_equal(got, want, "%s scale %r %g Msps: %s (thr %r)" % (fmt, scale, sps, name, float(thr)))
            n_cases += 1
            n_recs += len(want)
    return n_cases, n_recs


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("fmt", ["fc32", "mag2"])
def test_float_formats(fmt, fs):
    n_cases, n_recs = _run(fmt, None, fs, True)
    assert n_cases >= 40 and n_recs > 20


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("fmt", ["sc16", "sc8", "cu8"])
def test_integer_formats_every_scale(fmt, fs):
    for label, scale in E.scales(fmt):
        _run(fmt, scale, fs, label == "default")


@pytest.mark.parametrize("sps", [2, 4, 6, 8, 20])
def test_negzero_rise_in_a_quiet_body(sps):
    """thr 0.0 on |IQ|^2 input: pulses that rise at a -0.0 sample, the last sample of a body whose bit patterns are all
    negative (edge_cases.negzero_pulses).  The pass runs k_detect (not the one-launch pass) with chunks of several tiles,
    so that the rise's mask comes from the skipped body and not from a unit's exact head."""
    from gr_adsb_amd import _native
    x = E.negzero_pulses(sps)
    units, chunk = _native.plan_chunks(len(x) - (8 * sps - 1), 6 * 4)         # simlib.sim_run's default grid_max = 6
    assert units > 4 and chunk >= 2 * E.TILE, (units, chunk)
    want = C.canonical(x, sps, np.float32(0.0))
    assert len(want) >= 20
    got, _ = simlib.sim_canonical(1, x, sps * 1e6, 0.0)
    assert_recs_equal(got, want, "-0.0 rises, %d Msps" % sps)
