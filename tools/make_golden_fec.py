"""Container-only: generate tests/golden/g_fec.npz -- known answers of the REFERENCE decoder's Conservative error
correction (decoder.py:325-347 decode_packet up to the repair: decode_header, check_parity, correct_errors with
error_corr="Conservative", empty aircraft table) under both msg_filter values.  Data only: inputs (packed bits) and the
reference's outputs.

Rows: every single and adjacent-pair error position of valid DF 11 and DF 17/18/19 replies whose last bit is 0 and whose
last bit is 1 (the repairs that change the DF among them), address/parity formats with 1-2 errors, unknown DFs, 3-bit
errors, random bits, and the rows of g_parity.npz.

Outputs per msg_filter f in (all = "All Messages", es = "Extended Squitter Only"):
  passed_<f>   check_parity() or, when it fails, correct_errors() -- what decode_packet tests against 1
  bits_<f>     the payload after correct_errors() (packed like the input)
  df0_<f>      DF of the received bits; df1_<f>: DF of bits_<f> (decode_packet re-reads the header on success)
  plen_<f>     payload_length check_parity() chose (-1: none; correct_burst_errors then does nothing)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as R                     # noqa: E402
from gr_adsb_amd import modulator as M      # noqa: E402

FILTERS = (("all", "All Messages"), ("es", "Extended Squitter Only"))


def valid_frame(df, rng, last):
    """A valid reply of a parity/interrogator format whose last bit is `last`."""
    while True:
        f = M.make_frame(df, rng)
        if df == 19:                        # the decoder treats DF19 as a parity/interrogator format
            f[88:] = [(M.crc24(f[:88]) >> (23 - k)) & 1 for k in range(24)]
        if f[-1] == last:
            return f


def pad112(f, rng):
    bits = np.zeros(112, np.uint8)
    bits[:len(f)] = f
    if len(f) < 112:
        bits[len(f):] = rng.integers(0, 2, 112 - len(f))
    return bits


def main():
    rng = np.random.default_rng(20261015)
    rows = []
    for df in (11, 17, 18, 19):
        for last in (0, 1):
            f = valid_frame(df, rng, last)
            L = len(f)
            base = pad112(f, rng)
            for width in (1, 2):
                for i in range(L - width + 1):
                    g = base.copy()
                    g[i:i + width] ^= 1
                    rows.append(g)
    # repairs inside the DF field: a zero-syndrome word of any DF d, received with 1-2 errors in bits 0..4 as a DF the
    # device acts on (11 for a 56-bit word, 17/18/19 for a 112-bit one) -- the decoder's repair then turns it back into d
    for d in range(32):
        for L in (56, 112):
            for last in (0, 1):
                while True:
                    w = np.zeros(L, np.uint8)
                    w[:5] = [(d >> (4 - k)) & 1 for k in range(5)]
                    w[5:L - 24] = rng.integers(0, 2, L - 29)
                    w[L - 24:] = [(M.crc24(w[:L - 24]) >> (23 - k)) & 1 for k in range(24)]
                    if w[-1] == last:
                        break
                for width in (1, 2):
                    for i in range(5 - width + 1):
                        g = w.copy()
                        g[i:i + width] ^= 1
                        rx = int(g[:5] @ np.array([16, 8, 4, 2, 1]))
                        if rx != d and ((L == 56 and rx == 11) or (L == 112 and rx in (17, 18, 19))):
                            rows.append(pad112(g, rng))
    for df in (0, 4, 5, 16, 20, 21, 24):
        for _ in range(12):
            g = pad112(M.make_frame(df, rng), rng)
            i = int(rng.integers(0, 111))
            g[i:i + int(rng.integers(1, 3))] ^= 1
            rows.append(g)
    for df in sorted(set(range(32)) - {0, 4, 5, 11, 16, 17, 18, 19, 20, 21, 24}):
        for _ in range(3):
            g = rng.integers(0, 2, 112).astype(np.uint8)
            g[:5] = [(df >> (4 - k)) & 1 for k in range(5)]
            rows.append(g)
    for _ in range(120):
        df = int(rng.choice([11, 17, 18, 19]))
        g = pad112(valid_frame(df, rng, int(rng.integers(0, 2))), rng)
        g[rng.choice(56 if df == 11 else 112, 3, replace=False)] ^= 1
        rows.append(g)
    rows += list(rng.integers(0, 2, (200, 112)).astype(np.uint8))
    rows += list(np.unpackbits(np.load(os.path.join(ROOT, "tests", "golden", "g_parity.npz"))["bits"], axis=1)[:, :112])
    bits = np.array(rows, dtype=np.uint8)
    out = {"bits": np.packbits(bits, axis=1)}
    for tag, filt in FILTERS:
        dec = R.load_reference_decoder(filt, "Conservative", "None")
        passed = np.zeros(len(bits), np.int32)
        df0 = np.zeros(len(bits), np.int32)
        df1 = np.zeros(len(bits), np.int32)
        plen = np.zeros(len(bits), np.int32)
        after = np.zeros_like(bits)
        for i, b in enumerate(bits):
            dec.reset()
            dec.bits = b.astype(int)
            dec.datetime = ""; dec.snr = 0.0; dec.timestamp = 0.0
            dec.decode_header()
            df0[i] = dec.df
            p = dec.check_parity()
            if p == 0:
                p = dec.correct_errors()
            passed[i] = int(p == 1)
            plen[i] = dec.payload_length
            after[i] = np.asarray(dec.bits, dtype=np.uint8)
            df1[i] = int(after[i][:5] @ np.array([16, 8, 4, 2, 1]))
        out["passed_" + tag] = passed
        out["df0_" + tag] = df0
        out["df1_" + tag] = df1
        out["plen_" + tag] = plen
        out["bits_" + tag] = np.packbits(after, axis=1)
        print(filt, ": passed", int(passed.sum()), "repaired", int((after != bits).any(axis=1).sum()),
              "DF changed", int((df0 != df1).sum()))
    path = os.path.join(ROOT, "tests", "golden", "g_fec.npz")
    np.savez_compressed(path, **out)
    print(path, len(bits), "pdus")


if __name__ == "__main__":
    main()
