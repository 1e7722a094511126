"""Cost of the opt-in aircraft table (ADSB_FLAG_AIRCRAFT_TABLE): wall time per pass with and without the flag, for
device-resident complex64 and int8 streams of 2^30 samples at 8 Msps, at config3's density (6000 bursts/s) and in a dense
stream (60000 bursts/s).  Pipelined (three passes in flight, adsb_submit_format_device / adsb_wait: the bench's
arrangement) and blocking (adsb_process_format_device).  The two contexts alternate, repeats report the median.  Every
pass of the flagged context publishes its records into the same table (the same stream again: its addresses are known).
    python tools/aircraft_cost.py [--reps 5] [--out profiles/aircraft_cost.txt]      (GPU box only)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gr_adsb_amd import _native as N  # noqa: E402
from gr_adsb_amd import modulator as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fs", type=float, default=8e6)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stream(n, bursts):
    """complex64 IQ on the device ([n, 2] float32), made in blocks of 2^24 samples (synth_iq_torch per block, seeded)."""
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


say("fs %g Msps, ms per pass (median of %d alternating repeats); overhead = on / off - 1" % (a.fs / 1e6, a.reps))
say("%-5s %6s %7s %-10s %10s %10s %9s %8s %8s" % ("fmt", "log2n", "bursts", "mode", "off_ms", "table_ms", "overhead", "records",
                                                 "ap_known"))
for bursts in (6000.0, 60000.0):
    for log2n in (30,):
        n = 1 << log2n
        z = stream(n, bursts)
        for fmt_name, fmt in (("fc32", N.FMT_FC32), ("sc8", N.FMT_SC8)):
            data = z if fmt == N.FMT_FC32 else as_sc8(z)
            torch.cuda.synchronize()
            ctxs = [N.Context(a.fs, 0.01, flags=f) for f in (0, N.FLAG_AIRCRAFT_TABLE)]
            if fmt == N.FMT_SC8:
                for c in ctxs:
                    c.set_format_scale(fmt, 2.0 / 127.0)
            ptr = data.data_ptr()
            recs = [c.process_format_device(fmt, ptr, n) for c in ctxs]          # warm-up, and the records of both
            assert len(recs[0]) == len(recs[1])
            fixed = int(np.count_nonzero(recs[1]["flags"] & N.BURST_AP_KNOWN))
            steps = 12
            for mode, fn in (("pipelined", pipelined), ("blocking", blocking)):
                t = [[], []]
                for _ in range(a.reps):
                    for k in (0, 1):
                        t[k].append(fn(ctxs[k], fmt, ptr, n, steps))
                off, on = float(np.median(t[0])), float(np.median(t[1]))
                say("%-5s %6d %7d %-10s %10.4f %10.4f %8.2f%% %8d %8d" % (fmt_name, log2n, bursts, mode, off, on,
                                                                          100.0 * (on / off - 1.0), len(recs[0]), fixed))
            for c in ctxs:
                c.close()
            del data
        del z
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
