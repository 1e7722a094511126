"""Cost of carrying receiver streams across batch calls: adsb_process_stream_batch* against adsb_process_batch* over the same
chunks as fresh items.  Shape: 1024 streams x 2^16-sample uint8 IQ chunks at 2 Msps, 16 consecutive calls, the bench's burst
density; device entry points (chunks in HBM) and host entry points (chunks in pageable host memory).
The baseline is the fresh-item batch call on the PARENT commit's build (--parent-lib: its libadsb_hip.so), alternated with this
tree's build on one box: every round runs three fresh child processes -- parent build / batch, this build / batch, this build
/ stream batch -- and prints each one's median wall time per call; the run-to-run spread is the spread of those medians over
the rounds.  The file reports the measured stream / batch ratio, the per-call host time (wall time of a call, which ends in a
stream synchronise), and whether the parent's and this tree's batch times agree within the spread (the existing kernels are
untouched).  Every child runs under a time limit of its own; the first non-zero exit ends the run.
    python tools/stream_batch_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 5] [--out profiles/stream_batch_cost.txt]
(GPU box only.)"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--streams", type=int, default=1024)
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--calls", type=int, default=16)
ap.add_argument("--child", choices=["batch", "stream"], default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--child-timeout", type=int, default=240)
a = ap.parse_args()

FMT_CU8, FS, THR = 4, 2e6, 0.01
K, NS, CALLS = a.streams, 1 << a.log2n, a.calls


def child():
    """one process, one library: median wall ms per call of the device and the host entry point -> one JSON line"""
    import numpy as np
    import torch
    from gr_adsb_amd import modulator as M
    c = ctypes
    lib = c.CDLL(a.lib)
    vp, i32, i64 = c.c_void_p, c.c_int32, c.c_int64
    lib.adsb_create.argtypes = [c.c_double, c.c_float, c.c_int, c.c_uint32, c.POINTER(vp)]
    lib.adsb_destroy.argtypes = [vp]
    lib.adsb_destroy.restype = None
    lib.adsb_set_format_scale.argtypes = [vp, c.c_int, c.c_float]
    sig = [vp, c.c_int, vp, i32, vp, i32, vp, c.POINTER(i32), c.POINTER(i32)]
    names = ("adsb_process_batch_device", "adsb_process_batch") if a.child == "batch" else \
        ("adsb_process_stream_batch_device", "adsb_process_stream_batch")
    for nm in names:
        getattr(lib, nm).argtypes = sig
    if a.child == "stream":
        lib.adsb_streams_open.argtypes = [vp, i32]
        lib.adsb_stream_reset.argtypes = [vp, i32]
    h = vp()
    assert lib.adsb_create(FS, THR, 0, 0, c.byref(h)) == 0
    assert lib.adsb_set_format_scale(h, FMT_CU8, 2.0 / 255.0) == 0
    if a.child == "stream":
        assert lib.adsb_streams_open(h, K) == 0
    # a pool of 2^26 samples: stream i's call k reads samples [(i * CALLS + k) * NS, + NS) of it (modulo the pool)
    dev = torch.device("cuda:0")
    POOL, blk = 1 << 26, 1 << 24
    fc = torch.cat([M.synth_iq_torch(blk, FS, 1000.0, 100 + b, dev) for b in range(POOL // blk)])
    u8 = torch.clamp(torch.floor(fc * 63.75 + 128.0), 0, 255).to(torch.uint8).contiguous()
    del fc
    torch.cuda.synchronize()
    host = u8.cpu().numpy().reshape(-1)                       # pageable
    bases = {"device": u8.data_ptr(), "host": host.ctypes.data}
    dt = np.dtype([("data", "<u8"), ("n", "<i8"), ("w2", "<i8"), ("threshold", "<f4"), ("reserved", "<u4")])      # both item types
    out = np.empty(1 << 18, dtype=np.dtype([("w", "<u8", (4,))]))
    first = np.zeros(K + 1, dtype=np.int32)
    n_out, n_fb = i32(0), i32(0)

    def tables(base):
        tabs = []
        for k in range(CALLS):
            t = np.zeros(K, dtype=dt)
            start = ((np.arange(K, dtype=np.int64) * CALLS + k) * NS) % POOL
            t["data"] = base + 2 * start
            t["n"], t["threshold"] = NS, THR
            # adsb_batch_item.abs_offset / adsb_stream_item.{stream, flags}
            t["w2"] = (np.arange(K, dtype=np.int64) * CALLS + k) * NS if a.child == "batch" else np.arange(K, dtype=np.int64)
            tabs.append(t)
        return tabs

    res = {"what": a.child, "lib": a.lib}
    for where, fn in zip(("device", "host"), names):
        f = getattr(lib, fn)
        tabs = tables(bases[where])
        times, recs = [], 0
        for rep in range(3):                                   # the first sequence warms up (buffers grow), two are timed
            if a.child == "stream":
                for i in range(K):
                    lib.adsb_stream_reset(h, i)
            for k in range(CALLS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = f(h, FMT_CU8, vp(tabs[k].ctypes.data), K, vp(out.ctypes.data), len(out), vp(first.ctypes.data),
                       c.byref(n_out), c.byref(n_fb))
                dtm = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and n_fb.value == 0, (rc, n_fb.value)
                if rep > 0:
                    times.append(dtm)
                    recs += n_out.value
        res[where] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                      "records": recs}
    lib.adsb_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    import numpy as np
    here = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sides = [("this build, batch", here, "batch"), ("this build, stream batch", here, "stream")]
    if a.parent_lib:
        sides.insert(0, ("parent build, batch", a.parent_lib, "batch"))
    say("%d streams x 2^%d-sample uint8 IQ chunks, 2 Msps, %d consecutive calls; median wall ms per call (two timed sequences "
        "per process), %d rounds of fresh processes, the sides alternated" % (K, a.log2n, CALLS, a.rounds))
    med = {s[0]: {"device": [], "host": []} for s in sides}
    for r in range(a.rounds):
        for name, lib, what in sides:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", what, "--lib", lib,
                   "--streams", str(K), "--log2n", str(a.log2n), "--calls", str(CALLS)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                say("round %d, %s: exit %d -- stopping\n%s" % (r, name, p.returncode, p.stdout[-2000:]))
                return p.returncode
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for where in ("device", "host"):
                med[name][where].append(res[where]["median_ms"])
            say("round %d  %-26s device %8.3f ms (min %.3f max %.3f)   host %8.3f ms (min %.3f max %.3f)   records %d / %d" % (
                r, name, res["device"]["median_ms"], res["device"]["min_ms"], res["device"]["max_ms"], res["host"]["median_ms"],
                res["host"]["min_ms"], res["host"]["max_ms"], res["device"]["records"], res["host"]["records"]))
    say("")
    mid, spread = {}, {}
    for name, _, _ in sides:
        for where in ("device", "host"):
            v = med[name][where]
            mid[name, where] = float(np.median(v))
            spread[name, where] = (max(v) - min(v)) / mid[name, where]
            say("%-26s %-6s median of rounds %8.3f ms per call, run-to-run spread %.1f %% (%s)" % (
                name, where, mid[name, where], 100 * spread[name, where], " ".join("%.3f" % t for t in v)))
    say("")
    for where in ("device", "host"):
        b, s = mid["this build, batch", where], mid["this build, stream batch", where]
        say("%-6s entry point: stream batch / batch = %.3f  (%.3f ms against %.3f ms per call: +%.3f ms)" % (where, s / b, s, b, s - b))
        if a.parent_lib:
            pb = mid["parent build, batch", where]
            tol = max(spread["parent build, batch", where], spread["this build, batch", where])
            d = abs(b - pb) / pb
            say("%-6s entry point: batch on the parent build %.3f ms, on this build %.3f ms: %.1f %% apart, spread %.1f %% -> %s" % (
                where, pb, b, 100 * d, 100 * tol, "agree within the spread" if d <= tol else "DIFFER by more than the spread"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
