"""SURVEY.md §8f-1, downstream witness: PDUs built by the drop-in path (gr_adsb_amd.blocks.make_pdu from the
device code's bits, offsets and SNR inputs) are consumed by the UNMODIFIED reference decoder exactly like
the reference front end's own PDUs: same published messages, same aircraft table.  The reference's answers are stored
data (tests/refstore.py: its decoder's output is filed under the PDUs it was fed, so PDUs that differ from the reference's
have no answer); the device code is executed by the CPU emulator here and by the GPU in test_gpu_parity."""
import refstore


def test_reference_decoder_sees_identical_pdus(monkeypatch):
    import time
    # the reference decoder stamps wall-clock seconds into its aircraft table (decoder.py:424,433,1124): freeze
    # the clock so the two decoder runs below cannot straddle a second boundary
    monkeypatch.setattr(time, "time", lambda: 1.7e9)
    import simlib
    from gr_adsb_amd import blocks, _native
    from gr_adsb_amd import modulator as M
    R = refstore.harness()
    fs, thr, n = 2e6, 0.01, 1 << 16
    iq, truth = M.synth_iq(n, fs, 4000, seed=12, df_choices=(11, 17), df_weights=(0.3, 0.7), return_truth=True)
    x = M.mag2(iq)
    # (a) the reference front end -> PDUs exactly as its demod publishes them
    ref = R.run_reference(x, fs, thr)
    ref_pdus = [blocks.make_pdu(0.0, fs, int(o), s, b) for o, s, b in zip(ref["pdu_offsets"], ref["pdu_snr"], ref["pdu_bits"])]
    # (b) the device code (emulated) -> PDUs through the drop-in block's own builder
    recs, _ = simlib.sim_canonical(0, iq, fs, thr)
    dem = (recs["flags"] & 1) != 0
    snr = _native.snr_db(recs["peak"], recs["median"])
    bits = _native.unpack_bits(recs["bits"])[:, :112]
    our_pdus = [blocks.make_pdu(0.0, fs, int(o), s, b) for o, s, b in zip(recs["offset"][dem], snr[dem], bits[dem])]
    assert len(our_pdus) == len(ref_pdus) > 50
    m_ref, planes_ref = R.decode_all(ref_pdus)
    m_our, planes_our = R.decode_all(our_pdus)
    assert m_our == m_ref
    assert planes_our == planes_ref
    # sanity: the synthetic frames carry valid parity, so the decoder does decode aircraft from them
    assert len(planes_ref) > 10
    assert any(port == "decoded" for port, _ in m_ref)
