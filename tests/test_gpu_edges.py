"""The edge-case matrix of tests/edge_cases.py on the GPU, through the C ABI: every input format at every scale of the
generator (int8 / uint8 power-of-two scales run the dot-product instances k_detect<5|6, .>), at the four instantiated
rates and two run-time strides, host and device-resident entry points, bit for bit against the C oracle on the oracle's
|IQ|^2 of the same bytes.  |IQ|^2 calls of at most four units (kWaves) run as the one-launch pass k_pass_small; the
matrix's longer cases (the carrier over tiles, the -0.0 rises, lengths from 4097 samples up) and the streams below run
k_detect<1, .>.  Plus the -0.0 rises on chunks of several tiles, one stream per format long enough for the bulk pass at
thr <= 0 and one with more than 32 768 records and a carrier through k_longrun, and the fused path's confidence ratios
for the integer formats."""
import warnings

import numpy as np
import pytest

import edge_cases as E
from helpers import Golden, assert_recs_equal, large_golden_names, preamble_train_iq
from oracle import adsb_oracle as O
from oracle import c_oracle as C
from test_gpu_parity import native, torch_mod  # noqa: F401  (the module's fixtures)

pytestmark = pytest.mark.gpu

RATES = (2e6, 4e6, 8e6, 20e6, 6e6, 12e6)


def _dev(torch, data):
    """a device tensor of exactly the bytes of `data` (no padding behind the last sample)"""
    raw = np.ascontiguousarray(data).view(np.uint8)
    return torch.from_numpy(raw.copy()).to("cuda:0")


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("fmt", list(E.FORMATS))
def test_edge_matrix(native, torch_mod, fmt, fs):
    f = E.FORMATS[fmt][0]
    sps = int(fs // 1e6)
    ctx = native.Context(fs, 0.01)
    n_cases = n_recs = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, scale in E.scales(fmt):
            if scale is not None:
                ctx.set_format_scale(f, scale)
            full = label in (None, "default")
            for name, data, x, thr in E.cases(fmt, scale, sps, full=full):
                what = "%s scale %s %d Msps: %s (thr %r)" % (fmt, label, sps, name, float(thr))
                want = C.canonical(x, sps, thr)
                ctx.set_threshold(thr)
                before = ctx.stats()["longrun_calls"]
                assert_recs_equal(ctx.process_format(f, data), want, what + " host")
                if name == "carrier over tiles" and full:
                    assert ctx.stats()["longrun_calls"] > before, what + ": k_longrun did not run"
                n = len(x)
                if n == 0:
                    continue
                t = _dev(torch_mod, data)
                torch_mod.cuda.synchronize()
                assert_recs_equal(ctx.process_format_device(f, t.data_ptr(), n), want, what + " device")
                if full or name.startswith("thr"):
                    assert_recs_equal(ctx.wait(ctx.submit_format_device(f, t.data_ptr(), n)), want, what + " submitted")
                n_cases += 1
                n_recs += len(want)
    assert n_cases >= 40 and n_recs > 20
    ctx.close()


@pytest.mark.parametrize("fs", RATES)
def test_negzero_rise_in_a_quiet_body(native, torch_mod, fs):
    """thr 0.0 on |IQ|^2 input: pulses that rise at a -0.0 sample, the last sample of a body whose bit patterns are all
    negative (edge_cases.negzero_pulses), on a stream of four tiles per resident wavefront -- chunks of several tiles, so
    that the rise's mask comes from the skipped body and not from a unit's exact head.  k_detect<1, .> must run with that
    plan (detect_grid), not the one-launch pass."""
    sps = int(fs // 1e6)
    ctx = native.Context(fs, 0.0)
    ctx.process_mag2(np.zeros(1 << 20, np.float32))
    resident = torch_mod.cuda.get_device_properties(0).multi_processor_count * ctx.stats()["blocks_per_cu"] * 4
    x = E.negzero_pulses(sps, ntiles=max(64, 4 * resident + 6))
    n = len(x)
    units, chunk = native.plan_chunks(n - (8 * sps - 1), resident)
    assert units > 4 and chunk >= 2 * E.TILE, (units, chunk)
    want = C.canonical(x, sps, np.float32(0.0))
    assert len(want) > 1000
    assert_recs_equal(ctx.process_mag2(x), want, "-0.0 rises, %d Msps, host" % sps)
    assert ctx.stats()["detect_grid"] == (units + 3) // 4
    t = _dev(torch_mod, x)
    torch_mod.cuda.synchronize()
    assert_recs_equal(ctx.process_format_device(native.FMT_MAG2, t.data_ptr(), n), want, "-0.0 rises, %d Msps, device" % sps)
    ctx.close()


def _large_inputs(fmt, n, sps):
    """(data, x, scale) of a bare-preamble train over n samples in the format (a preamble every 32 symbols: a record every
    64 symbols after the gate) with a 5000-sample carrier in the middle (k_longrun), default scales"""
    iq = preamble_train_iq(n, sps=sps)
    iq[n // 2:n // 2 + 5000] = np.complex64(1.0)
    scale = E.FORMATS[fmt][1]
    if fmt in ("fc32", "mag2"):
        x = O.mag2(iq)
        return (iq if fmt == "fc32" else x), x, None
    k = {"sc16": 16384.0, "sc8": 64.0, "cu8": 64.0}[fmt]
    i = np.rint(iq.real.astype(np.float64) * k).astype(np.int64)
    q = np.rint(iq.imag.astype(np.float64) * k).astype(np.int64)
    if fmt == "sc16":
        data = np.empty(2 * n, dtype=np.int16)
        data[0::2], data[1::2] = i, q
        return data, O.mag2_iq16(data, scale), scale
    return E.encode(fmt, np.clip(i, -128, 127), np.clip(q, -128, 127), scale) + (scale,)


@pytest.mark.parametrize("fmt", list(E.FORMATS))
def test_large_streams(native, torch_mod, fmt):
    """2^22 samples at thr -1 and 0.0 (every sample above, the zero history in front of the stream included: no rise and
    no fall, nothing for k_longrun to finish -- the bulk pass must find no pulse at all) and 6 * 2^20 samples with more
    than 32 768 records and a carrier that only k_longrun finishes, host and
    device-resident."""
    f = E.FORMATS[fmt][0]
    ctx = native.Context(2e6, 0.01)
    n = (1 << 22) + 3
    data, x, scale = _large_inputs(fmt, n, 2)
    if scale is not None:
        ctx.set_format_scale(f, scale)
    for thr in (np.float32(-1.0), np.float32(0.0)):
        ctx.set_threshold(thr)
        want = C.canonical(x, 2, thr)
        assert_recs_equal(ctx.process_format(f, data), want, "%s 2^22 thr %r" % (fmt, float(thr)))
    n = 6 << 20
    data, x, scale = _large_inputs(fmt, n, 2)
    ctx.set_threshold(0.01)
    want = C.canonical(x, 2, np.float32(0.01))
    assert len(want) > 32768, len(want)
    before = ctx.stats()["longrun_calls"]
    assert_recs_equal(ctx.process_format(f, data), want, fmt + " dense host")
    assert ctx.stats()["longrun_calls"] > before, fmt + ": the carrier did not reach k_longrun"
    t = _dev(torch_mod, data)
    torch_mod.cuda.synchronize()
    assert_recs_equal(ctx.process_format_device(f, t.data_ptr(), n), want, fmt + " dense device")
    assert_recs_equal(ctx.wait(ctx.submit_format_device(f, t.data_ptr(), n)), want, fmt + " dense submitted")
    ctx.close()


@pytest.mark.parametrize("name", large_golden_names())
def test_fused_path_confidence_int8_goldens(native, name):
    """ADSB_FLAG_CONFIDENCE on int8 input (k_confidence<3>, and k_confidence<3> behind k_detect<5, .> at a power-of-two
    scale): the ratios of every PDU equal the reference's bit_confidence bits stored with the L*.npz goldens."""
    g = Golden(name)
    ctx = native.Context(g.fs, g.thr, flags=native.FLAG_CONFIDENCE)
    ctx.set_format_scale(native.FMT_SC8, float(g.scale))
    recs = ctx.process_format(native.FMT_SC8, g.iq8)
    dem = (recs["flags"] & 1) != 0
    assert dem.sum() > 100
    ratio = ctx.last_confidence()
    assert ratio.shape == (len(recs), 112)
    assert np.array_equal(native.confidence_db(ratio[dem]).view(np.uint32), g.get("single", "pdu_conf_bits"))
    assert not np.any(ratio[~dem].view(np.uint32))
    ctx.close()


@pytest.mark.parametrize("fmt,scale", [("sc8", 2.0 ** -6), ("sc8", 2.0 / 127.0), ("cu8", 2.0 ** -7), ("cu8", 2.0 / 255.0),
                                       ("sc16", 2.0 / 32767.0)])
@pytest.mark.parametrize("fs", [2e6, 8e6, 6e6])
def test_fused_path_confidence_integer_formats(native, fmt, scale, fs):
    """ADSB_FLAG_CONFIDENCE ratios on integer input (k_confidence<2|3|4>) against the oracle's demod.py:97-101 ratios of the
    oracle's |IQ|^2 of the same bytes, bit for bit (NaN where the oracle has NaN)."""
    from gr_adsb_amd import modulator as M
    f = E.FORMATS[fmt][0]
    sps = int(fs // 1e6)
    iq = M.synth_iq(1 << 16, fs, 6000, seed=40 + sps, noise_power=2e-3, amp2_range=(0.05, 1.0))
    scale = float(np.float32(scale))
    if fmt == "sc16":
        q = M.quantize_iq16(iq, full_scale=2.0)
        x = O.mag2_iq16(q, scale)
    else:
        q = M.quantize_iq8(iq, full_scale=2.0, offset_binary=fmt == "cu8")
        x = O.mag2_iq8(q, scale, fmt == "cu8")
    thr = np.float32(0.01)
    ctx = native.Context(fs, thr, flags=native.FLAG_CONFIDENCE)
    ctx.set_format_scale(f, scale)
    recs = ctx.process_format(f, q)
    assert_recs_equal(recs, C.canonical(x, sps, thr), "%s %r" % (fmt, scale))
    o = O.run_stream(x, fs, thr)
    dem = (recs["flags"] & 1) != 0
    got, want = ctx.last_confidence()[dem], o["pdu_ratio"]
    assert len(want) > 10 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))
    ctx.close()
