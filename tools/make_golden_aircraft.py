"""Container-only: generate tests/golden/g_aircraft.npz -- known answers of the REFERENCE decoder's aircraft table
(decoder.py:576-665 check_parity of the address/parity formats, update_plane from decode_message / decode_me) for
sequences of PDUs fed through its decode_packet, under msg_filter "All Messages" / "Extended Squitter Only" and error_corr
"None" / "Conservative".  Data only: inputs (packed bits, sequence ids) and the reference's outputs.

Each sequence goes to a fresh decoder, one PDU after the other.  Rows cover every announcing and non-announcing
DF/TC/CF/AF/ST class; address/parity (AP) replies of every AP format before, right after, later than and never after their
address's announcement; and crafted rows for the Conservative repair: AP replies whose (AA, last bit) is an error pattern's
key or misses it by the last bit, repairs that turn DF 16/20/21 into 17/18/19, and DF 11/17/19 replies whose repair changes
the format (the device leaves those raw).

Outputs per configuration <m>_<e> (m: all / es, e: none / cons):
  passed_<m>_<e>  1 if check_parity() or, when it fails, correct_errors() accepted the PDU (what decode_packet tests)
  added_<m>_<e>   the address the PDU added to plane_dict (int), -1 if none (the key "" is not an address: ignored)
  raised_<m>_<e>  1 if decode_packet raised (the table state is what plane_dict holds afterwards)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as R                     # noqa: E402
from gr_adsb_amd import modulator as M      # noqa: E402

CONFIGS = (("all_none", "All Messages", "None"), ("all_cons", "All Messages", "Conservative"),
           ("es_none", "Extended Squitter Only", "None"), ("es_cons", "Extended Squitter Only", "Conservative"))
AP_DFS = (0, 4, 5, 16, 20, 21, 24)


def ib(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def pad112(f, rng):
    b = np.zeros(112, np.uint8)
    b[:len(f)] = f
    if len(f) < 112:
        b[len(f):] = rng.integers(0, 2, 112 - len(f))
    return b


def pi_reply(df, aa, rng, sub=0, tc=11, st=1):
    """A valid parity/interrogator reply: DF 11 (56 bits), or DF 17/18/19 with CF/AF `sub`, TC, ST."""
    L = 56 if df == 11 else 112
    f = np.zeros(L, np.uint8)
    f[:5] = ib(df, 5)
    f[5:8] = ib(sub, 3)
    f[8:32] = ib(aa, 24)
    if L == 112:
        f[32:37] = ib(tc, 5)
        f[37:40] = ib(st, 3)
        f[40:88] = rng.integers(0, 2, 48)
    f[L - 24:] = ib(M.crc24(f[:L - 24]), 24)
    return pad112(f, rng)


def ap_reply(df, aa, rng):
    """An address/parity reply whose AA is `aa`."""
    return pad112(M.make_frame(df, rng, icao=aa), rng)


def syndrome(bits, L):
    return M.crc24(bits[:L - 24]) ^ int("".join(map(str, bits[L - 24:L])), 2)


def pattern(L, i, w):
    e = np.zeros(L, np.uint8)
    e[i:i + w] = 1
    return e


def ap_on_pattern(df, i, w, rng, match=True, fix=None):
    """An AP reply whose AA is the syndrome of the error pattern (i, w) -- the decoder's repair key is (AA, last bit) --
    with the pattern's last bit (match) or the other one.  fix(bits) -> bool: extra condition on the repaired reply."""
    L = 56 if df in (0, 4, 5) else 112
    e = pattern(L, i, w)
    s = syndrome(e, L)
    for _ in range(100000):
        f = np.zeros(L, np.uint8)
        f[:5] = ib(df, 5)
        f[5:L - 24] = rng.integers(0, 2, L - 29)
        f[L - 24:] = ib(M.crc24(f[:L - 24]) ^ s, 24)
        if (f[-1] == e[-1]) != match:
            continue
        if fix is not None and not fix(f ^ e):
            continue
        return pad112(f, rng)
    raise RuntimeError("no reply found")


def raw_fec_df(d, rx, L, rng, fix=None):
    """A zero-syndrome L-bit word of DF d with last bit 0, received with the DF bits flipped into rx: the decoder's repair
    turns it back into d (a format change: the device leaves it raw)."""
    diff = d ^ rx
    pos = [k for k in range(5) if (diff >> (4 - k)) & 1]
    assert len(pos) in (1, 2) and (len(pos) == 1 or pos[1] == pos[0] + 1)
    for _ in range(100000):
        w = np.zeros(L, np.uint8)
        w[:5] = ib(d, 5)
        w[5:L - 24] = rng.integers(0, 2, L - 29)
        w[L - 24:] = ib(M.crc24(w[:L - 24]), 24)
        if w[-1] != 0:
            continue
        full = pad112(w, rng)
        if fix is not None and not fix(full):
            continue
        full[pos] ^= 1
        return full
    raise RuntimeError("no word found")


def field(b, lo, n):
    return int("".join(map(str, b[lo:lo + n])), 2)


def sequences(rng):
    seqs = []
    addr = iter(rng.permutation(np.arange(0x100000, 0xFFFFFF))[:4000].tolist())
    # 1. every announcing / non-announcing class, each followed by an AP reply of its address (and one before it)
    classes = [(11, 0, 0, 0)]
    for tc in range(32):
        for st in ((1, 2, 3, 4, 0) if tc == 19 else (int(rng.integers(0, 8)),)):
            classes.append((17, int(rng.integers(0, 8)), tc, st))
    for cf in range(8):
        for tc in (1, 5, 11, 19, 22):
            classes.append((18, cf, tc, 1))
    for af in range(8):
        for tc in (3, 12, 19, 28):
            classes.append((19, af, tc, 2))
    for df, sub, tc, st in classes:
        a = next(addr)
        apdf = AP_DFS[len(seqs) % len(AP_DFS)]
        seqs.append([ap_reply(apdf, a, rng), pi_reply(df, a, rng, sub, tc, st), ap_reply(apdf, a, rng),
                     ap_reply(AP_DFS[(len(seqs) + 3) % 7], a, rng)])
    # 2. AP replies of every format: before, right after, later than and never after an announcement
    for apdf in AP_DFS:
        a, b = next(addr), next(addr)
        seq = [ap_reply(apdf, a, rng), pi_reply(17, a, rng, tc=4)]
        seq += [ap_reply(apdf, a, rng), ap_reply(apdf, b, rng), pi_reply(11, next(addr), rng)]
        seq += [ap_reply(apdf, a, rng), ap_reply(apdf, b, rng)]
        seqs.append(seq)
        # a damaged announcement (parity fails, no repair) does not announce; a damaged AP reply misses its address
        bad = pi_reply(17, b, rng, tc=12)
        bad[60] ^= 1
        bad[70] ^= 1
        bad[90] ^= 1
        dam = ap_reply(apdf, a, rng)
        dam[8] ^= 1
        dam[30] ^= 1
        dam[45] ^= 1
        seqs.append([pi_reply(11, a, rng), bad, ap_reply(apdf, b, rng), dam, ap_reply(apdf, a, rng)])
    # 3. the Conservative repair of AP replies: pattern keys with the matching and the other last bit
    for apdf in AP_DFS:
        L = 56 if apdf in (0, 4, 5) else 112
        for i, w in ((L - 1, 1), (L - 2, 2), (L - 2, 1), (40, 1), (40, 2), (7, 1), (20, 2)):
            f = ap_on_pattern(apdf, i, w, rng, match=True)
            g = ap_on_pattern(apdf, i, w, rng, match=False)
            seqs.append([f, g, f.copy(), ap_reply(apdf, syndrome(f, L), rng)])
    # conditional repairs into DF 17/18/19 (announcing and not), and DF 24 / unknown DFs after the repair
    conds = [(16, 4, 1), (16, 3, 1), (16, 3, 2), (20, 2, 2), (21, 2, 1), (21, 2, 2), (16, 1, 1), (20, 1, 2), (4, 2, 1),
             (5, 3, 1), (0, 0, 1)]
    for apdf, i, w in conds:
        for tc in (11, 7):
            fix = (lambda r, tc=tc: field(r, 32, 5) == tc and field(r, 5, 3) == 0)
            f = ap_on_pattern(apdf, i, w, rng, match=True, fix=fix)
            L = 56 if apdf in (0, 4, 5) else 112
            rep = f.copy()
            rep[i:i + w] ^= 1
            B = field(rep, 8, 24)
            aa = syndrome(f, L)
            # unknown AA: repaired, announces B; then replies of B and of AA
            seqs.append([f, ap_reply(20, B, rng), ap_reply(apdf, aa, rng), ap_reply(4, B, rng)])
            # known AA: no repair, nothing announced
            seqs.append([pi_reply(11, aa, rng), f, ap_reply(21, B, rng)])
            # the same reply twice: the second sees the first's announcement
            seqs.append([f, f.copy(), ap_reply(5, aa, rng)])
    # 4. DF 11/17/19 replies whose repair changes the format: 11 <-> 19 (length changes), 17 -> 16 (an AP result)
    for d, rx, L in ((19, 11, 56), (11, 19, 112), (16, 17, 112), (19, 17, 112), (17, 16, 112)):
        for k in range(3):
            fix = None
            if d == 19:
                fix = (lambda r: field(r, 5, 3) == 0 and field(r, 32, 5) in (2, 10, 15))
            r = raw_fec_df(d, rx, L, rng, fix=fix)
            fixed = r.copy()
            diff = d ^ rx
            for q in range(5):
                if (diff >> (4 - q)) & 1:
                    fixed[q] ^= 1
            B = field(fixed, 8, 24)
            seqs.append([r, ap_reply(AP_DFS[k], B, rng), ap_reply(16, B, rng)])
    # 5. noise: random bits of every DF, and mixed traffic of a few aircraft
    noise = [rng.integers(0, 2, 112).astype(np.uint8) for _ in range(300)]
    seqs.append(noise)
    planes = [next(addr) for _ in range(6)]
    mix = []
    for _ in range(150):
        a = planes[int(rng.integers(0, 6))]
        kind = int(rng.integers(0, 5))
        if kind == 0:
            mix.append(pi_reply(int(rng.choice([11, 17, 18, 19])), a, rng, sub=int(rng.choice([0, 0, 1, 6, 2])),
                                tc=int(rng.integers(0, 32)), st=int(rng.integers(0, 5))))
        elif kind == 4:
            mix.append(rng.integers(0, 2, 112).astype(np.uint8))
        else:
            mix.append(ap_reply(int(rng.choice(AP_DFS)), a, rng))
    seqs.append(mix)
    return seqs


def run(dec, rows):
    """decode_packet on each row; -> passed, added, raised per row."""
    passed, added, raised = [], [], []
    for b in rows:
        got = {}
        cp, ce = dec.check_parity, dec.correct_errors

        def check(_cp=cp):
            got["p"] = _cp()
            return got["p"]

        def corr(_ce=ce):
            got["c"] = _ce()
            return got["c"]
        dec.check_parity, dec.correct_errors = check, corr
        before = set(dec.plane_dict)
        r = 0
        try:
            dec.decode_packet(({"timestamp": 0.0, "snr": 0.0}, np.array(b, dtype=np.uint8)))   # a u8vector: NumPy
        except Exception:
            r = 1
        dec.check_parity, dec.correct_errors = cp, ce
        new = [k for k in set(dec.plane_dict) - before if k != ""]
        assert len(new) <= 1
        passed.append(int(got.get("p") == 1 or got.get("c") == 1))
        added.append(int(new[0], 16) if new else -1)
        raised.append(r)
    return passed, added, raised


def main():
    rng = np.random.default_rng(20261016)
    seqs = sequences(rng)
    bits = np.array([b for s in seqs for b in s], dtype=np.uint8)
    seq = np.array([i for i, s in enumerate(seqs) for _ in s], dtype=np.int32)
    out = {"bits": np.packbits(bits, axis=1), "seq": seq}
    for tag, filt, corr in CONFIGS:
        passed, added, raised = [], [], []
        for s in seqs:
            dec = R.load_reference_decoder(filt, corr, "None")
            p, a, r = run(dec, s)
            passed += p
            added += a
            raised += r
        out["passed_" + tag] = np.array(passed, np.int32)
        out["added_" + tag] = np.array(added, np.int64)
        out["raised_" + tag] = np.array(raised, np.int32)
        print(tag, "passed", sum(passed), "added", sum(x >= 0 for x in added), "raised", sum(raised))
    path = os.path.join(ROOT, "tests", "golden", "g_aircraft.npz")
    np.savez_compressed(path, **out)
    print(path, len(bits), "pdus in", len(seqs), "sequences")


if __name__ == "__main__":
    main()
