"""Cost of the opt-in decode step (ADSB_FLAG_DECODE).
  passes: wall time per pass of 2^30 samples at 8 Msps (config3's density, 6000 bursts/s), device-resident complex64 and
    int8, with the aircraft table alone and with the table plus the decode step; pipelined (three passes in flight,
    adsb_submit_format_device / adsb_wait: the bench's arrangement) and blocking (adsb_process_format_device).  The two
    contexts alternate, repeats report the median.
  pdus: adsb_decode_pdus throughput for 10^4 - 10^6 PDUs (DF 17 identifications, positions and velocities with valid
    parity) over 5 aircraft and over as many aircraft as PDUs.
  reference: the unmodified reference decoder's decode_packet per PDU on one CPU thread, for context (only where the
    reference exists: --reference, never on the GPU box).
    python tools/decode_cost.py [--reps 5] [--out FILE]            (GPU box)
    python tools/decode_cost.py --reference [--out FILE]           (where the reference exists)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from gr_adsb_amd import _native as N  # noqa: E402
from gr_adsb_amd import modulator as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fs", type=float, default=8e6)
ap.add_argument("--reference", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


# x^j mod G for the message bits: the parity of 88 bits is the XOR of the rows of the set bits
_G = 0x1FFF409
_R = []
for i in range(88):
    e = np.zeros(88, np.uint8)
    e[i] = 1
    _R.append(M.crc24(e))
_R = np.array(_R, np.uint32)


def pdus(n, n_air, seed=1):
    """n DF 17 PDUs (packed, [n, 14]) of n_air aircraft: identifications, positions and velocities with valid parity, and
    their timestamps (one every millisecond)."""
    rng = np.random.default_rng(seed)
    bits = np.zeros((n, 112), np.uint8)
    bits[:, :5] = [1, 0, 0, 0, 1]
    aa = rng.integers(0x100000, 0x1000000, n_air)[rng.integers(0, n_air, n)] if n_air < n else rng.permutation(1 << 24)[:n]
    bits[:, 8:32] = (aa[:, None] >> np.arange(23, -1, -1)) & 1
    kind = rng.integers(0, 4, n)
    tc = np.where(kind == 0, 4, np.where(kind == 3, 19, 11))
    bits[:, 32:37] = (tc[:, None] >> np.arange(4, -1, -1)) & 1
    bits[:, 37:88] = rng.integers(0, 2, (n, 51))
    vel = kind == 3
    bits[vel, 37:40] = [0, 0, 1]
    bits[:, 53] = np.arange(n) & 1
    par = np.bitwise_xor.reduce(np.where(bits[:, :88].astype(bool), _R[None, :], 0), axis=1)
    bits[:, 88:] = (par[:, None] >> np.arange(23, -1, -1)) & 1
    return np.packbits(bits, axis=1), 1760000000.0 + 1e-3 * np.arange(n)


if a.reference:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_harness as R
    say("reference decoder (decode_packet, one CPU thread), us per PDU")
    for n_air in (5, 2000):
        b14, ts = pdus(20000, n_air)
        b = np.unpackbits(b14, axis=1)
        dec = R.load_reference_decoder("All Messages", "None", "None")
        t0 = time.perf_counter()
        for i in range(len(b)):
            dec.decode_packet(({"timestamp": float(ts[i]), "snr": 10.0}, b[i].copy()))
        say("%6d aircraft  %8.1f us/PDU" % (n_air, (time.perf_counter() - t0) / len(b) * 1e6))
else:
    import torch
    dev = torch.device("cuda:0")

    def stream(n, bursts):
        z = torch.empty((n, 2), dtype=torch.float32, device=dev)
        blk = 1 << 24
        for b in range(0, n, blk):
            m = min(blk, n - b)
            z[b:b + m] = M.synth_iq_torch(m, a.fs, bursts, 1000 + b // blk, dev)
        return z

    def as_sc8(z):
        return torch.clamp(torch.round(z.reshape(-1) * (127.0 / 2.0)), -128, 127).to(torch.int8)

    def pipelined(ctx, fmt, ptr, n, steps):
        tickets = []
        t0 = time.perf_counter()
        for _ in range(steps):
            if len(tickets) == 3:
                ctx.wait(tickets.pop(0), fetch=False)
            tickets.append(ctx.submit_format_device(fmt, ptr, n))
        while tickets:
            ctx.wait(tickets.pop(0), fetch=False)
        return (time.perf_counter() - t0) / steps * 1e3

    def blocking(ctx, fmt, ptr, n, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.process_format_device(fmt, ptr, n, fetch=False)
        return (time.perf_counter() - t0) / steps * 1e3

    T, D = N.FLAG_AIRCRAFT_TABLE, N.FLAG_AIRCRAFT_TABLE | N.FLAG_DECODE
    say("passes: fs %g Msps, ms per pass (median of %d alternating repeats); overhead = decode / table - 1" % (a.fs / 1e6, a.reps))
    say("%-5s %6s %7s %-10s %10s %10s %9s %8s %8s" % ("fmt", "log2n", "bursts", "mode", "table_ms", "decode_ms", "overhead",
                                                     "records", "decoded"))
    n = 1 << 30
    z = stream(n, 6000.0)
    for fmt_name, fmt in (("fc32", N.FMT_FC32), ("sc8", N.FMT_SC8)):
        data = z if fmt == N.FMT_FC32 else as_sc8(z)
        torch.cuda.synchronize()
        ctxs = [N.Context(a.fs, 0.01, flags=f) for f in (T, D)]
        if fmt == N.FMT_SC8:
            for c in ctxs:
                c.set_format_scale(fmt, 2.0 / 127.0)
        ptr = data.data_ptr()
        recs = [c.process_format_device(fmt, ptr, n) for c in ctxs]
        assert recs[0].tobytes() == recs[1].tobytes()
        ndec = int((ctxs[1].last_decoded()["port"] == N.DEC_DECODED).sum())
        for mode, fn in (("pipelined", pipelined), ("blocking", blocking)):
            t = [[], []]
            for _ in range(a.reps):
                for k in (0, 1):
                    t[k].append(fn(ctxs[k], fmt, ptr, n, 12))
            off, on = float(np.median(t[0])), float(np.median(t[1]))
            say("%-5s %6d %7d %-10s %10.4f %10.4f %8.2f%% %8d %8d" % (fmt_name, 30, 6000, mode, off, on, 100.0 * (on / off - 1.0),
                                                                      len(recs[0]), ndec))
        for c in ctxs:
            c.close()
        del data
    del z
    torch.cuda.empty_cache()
    say("")
    say("adsb_decode_pdus: one call per batch, median of %d (a fresh decoder state each time: adsb_reset)" % a.reps)
    say("%8s %9s %10s %12s" % ("pdus", "aircraft", "ms/call", "Mpdu/s"))
    c = N.Context(2e6, 0.0, flags=D)
    for npdu in (10 ** 4, 10 ** 5, 10 ** 6):
        for n_air in (5, npdu):
            b14, ts = pdus(npdu, n_air)
            t = []
            for _ in range(a.reps):
                c.reset()
                t0 = time.perf_counter()
                c.decode_pdus(b14, ts)
                t.append(time.perf_counter() - t0)
            ms = float(np.median(t)) * 1e3
            say("%8d %9d %10.3f %12.2f" % (npdu, n_air, ms, npdu / ms / 1e3))
    c.close()
if a.out:
    mode = "a" if os.path.exists(a.out) and a.reference else "w"
    with open(a.out, mode) as f:
        f.write("\n".join(lines) + "\n")
