"""Cost of a batch of independent streams: N receivers' chunks as N submitted passes against ONE adsb_process_batch_device call.
  side A, what the library offered before: every item through adsb_submit_format_device / adsb_wait, three in flight;
  side B: one adsb_process_batch_device call (k_batch: one workgroup per item; k_batch_pack).
Shapes {64, 1024, 4096} items x {2^14, 2^16, 2^20} samples (those over 2^32 bytes skipped) and, for the crossover with few long
items, {16, 32} x 2^20, complex64 and uint8 IQ, 2 Msps, the
bench's burst density; inputs device-resident (windows of one pool, consecutive where the pool holds the batch).  One process;
every shape is warmed up on both sides, then the sides alternate and EVERY repeat is printed: wall time per batch around a call
sequence that ends in a device synchronise, Gsamples/s, the records delivered, n_fallback.  Both sides call the C ABI through
ctypes with tables built beforehand (what a C client pays).
    python tools/batch_cost.py [--reps 5] [--out FILE]            (GPU box only)"""
import argparse
import ctypes
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
ap.add_argument("--fs", type=float, default=2e6)
ap.add_argument("--bursts-per-s", type=float, default=1000.0)
ap.add_argument("--pool-log2", type=int, default=28)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda:0")
POOL = 1 << a.pool_log2
blk = 1 << 24
fc = torch.cat([M.synth_iq_torch(blk, a.fs, a.bursts_per_s, 100 + b, dev) for b in range(POOL // blk)])      # float32 [POOL, 2]
u8 = torch.clamp(torch.floor(fc * 63.75 + 128.0), 0, 255).to(torch.uint8)                                       # cu8, full scale 2
torch.cuda.synchronize()
pools = {N.FMT_FC32: fc, N.FMT_CU8: u8}
names = {N.FMT_FC32: "complex64", N.FMT_CU8: "uint8"}
say("fs %g, %g bursts/s, pool 2^%d samples; wall per batch in ms (every repeat), median Gsamples/s" % (a.fs, a.bursts_per_s, a.pool_log2))

i32 = ctypes.c_int32
for fmt in (N.FMT_FC32, N.FMT_CU8):
    bps = N.FMT_BYTES[fmt]
    base = pools[fmt].data_ptr()
    for k in (16, 32, 64, 1024, 4096):
        for log2n in ((20,) if k < 64 else (14, 16, 20)):
            n = 1 << log2n
            if k * n * bps > (1 << 32):
                say("%-9s %5d x 2^%d: skipped (over 2^32 bytes)" % (names[fmt], k, log2n))
                continue
            ca, cb = N.Context(a.fs, 0.01), N.Context(a.fs, 0.01)
            for c in (ca, cb):
                c.set_format_scale(N.FMT_CU8, 2.0 / 255.0)
            ptrs = [base + ((i * n) % POOL) * bps for i in range(k)]
            table = np.zeros(k, dtype=N.BATCH_ITEM_DTYPE)
            table["data"], table["n"], table["threshold"] = ptrs, n, 0.01
            table["abs_offset"] = np.arange(k, dtype=np.int64) * n
            out = np.empty(max(1 << 16, k * n // 500), dtype=N.BURST_DTYPE)
            first = np.zeros(k + 1, dtype=np.int32)
            n_out, n_fb, tk = i32(0), i32(0), i32(0)
            vp = [ctypes.c_void_p(p) for p in ptrs]
            offs = [int(o) for o in table["abs_offset"]]
            lib, ha, hb = ca.lib, ca._h, cb._h

            def side_a():
                pend, tot = [], 0
                for i in range(k):
                    rc = lib.adsb_submit_format_device(ha, fmt, vp[i], n, offs[i], ctypes.byref(tk))
                    assert rc == 0, rc
                    pend.append(tk.value)
                    if len(pend) == 3:
                        assert lib.adsb_wait(ha, pend.pop(0), None, 0, ctypes.byref(n_out)) == 0
                        tot += n_out.value
                while pend:
                    assert lib.adsb_wait(ha, pend.pop(0), None, 0, ctypes.byref(n_out)) == 0
                    tot += n_out.value
                return tot, 0

            def side_b():
                rc = lib.adsb_process_batch_device(hb, fmt, ctypes.c_void_p(table.ctypes.data), k, ctypes.c_void_p(out.ctypes.data),
                                                   len(out), ctypes.c_void_p(first.ctypes.data), ctypes.byref(n_out), ctypes.byref(n_fb))
                assert rc == 0, (rc, n_out.value)
                return n_out.value, n_fb.value

            def timed(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, r

            for _ in range(2):
                ra, rb = side_a(), side_b()
            assert ra[0] == rb[0], (ra, rb)              # the same records either way (bytes: tests/test_gpu_batch.py)
            ta, tb = [], []
            for _ in range(a.reps):
                ta.append(timed(side_a)[0])
                tb.append(timed(side_b)[0])
            ma, mb = float(np.median(ta)), float(np.median(tb))
            say("%-9s %5d x 2^%d  A submit/wait x3: %s  -> %7.1f Gs/s | B batch: %s  -> %7.1f Gs/s | B/A speed %5.2fx  spread A %.0f%% B %.0f%%  records %d  n_fallback %d" % (
                names[fmt], k, log2n, " ".join("%8.3f" % t for t in ta), k * n / ma / 1e6, " ".join("%8.3f" % t for t in tb),
                k * n / mb / 1e6, ma / mb, 100 * (max(ta) - min(ta)) / ma, 100 * (max(tb) - min(tb)) / mb, rb[0], rb[1]))
            ca.close()
            cb.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
