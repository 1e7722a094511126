"""Cost of one decoder behind every receiver stream (ADSB_FLAG_STREAM_DECODE) on the workload of tools/stream_batch_cost.py:
1024 streams x 2^16-sample uint8 IQ chunks at 2 Msps, 16 consecutive calls, the bench's burst density.  Four measurements,
each the median wall time of a call (a call ends in a stream synchronise) in a fresh child process:
  (a) adsb_process_stream_batch_device / adsb_process_stream_batch on a context WITH the flag (this build);
  (b) the same calls on a context without the flag (this build);
  (c) the same on the PARENT commit's build (--parent-lib: its libadsb_hip.so), run TWICE per round: the run-to-run spread
      that (b) is held against;
  (d) what a user has to do without the flag: the records of one call decoded stream by stream with adsb_decode_pdus on an
      ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE context -- ONE context here (a fleet that wanted its streams apart would need
      one 1.5 GiB context per stream); the time is the sum of the per-stream calls of one stream-batch call.
The file states (a) / (b), (d) / ((a) - (b)) and whether (b) and (c) agree within the spread of (c)'s two runs, as measured.
Every child runs under a time limit of its own; the first non-zero exit ends the run.
    python tools/stream_decode_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 3] [--out profiles/stream_decode_cost.txt]
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--streams", type=int, default=1024)
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--calls", type=int, default=16)
ap.add_argument("--child", choices=["stream", "fleet", "pdus"], default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--extra-flags", type=int, default=0)      # child "fleet": more context flags (tools/expire_cost.py: 2048)
ap.add_argument("--child-timeout", type=int, default=240)
a = ap.parse_args()

FMT_CU8, FS, THR = 4, 2e6, 0.01
FLAG_TABLE, FLAG_DECODE, FLAG_STREAM_DECODE = 256, 512, 1024
K, NS, CALLS = a.streams, 1 << a.log2n, a.calls


def child():
    """one process, one library -> one JSON line.  stream / fleet: median wall ms per call of the device and the host entry
    point; pdus: median, over the calls, of the time the per-stream adsb_decode_pdus calls of one call's records take."""
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
    names = ("adsb_process_stream_batch_device", "adsb_process_stream_batch")
    for nm in names:
        getattr(lib, nm).argtypes = sig
    lib.adsb_streams_open.argtypes = [vp, i32]
    lib.adsb_stream_reset.argtypes = [vp, i32]
    h = vp()
    assert lib.adsb_create(FS, THR, 0, (FLAG_STREAM_DECODE | a.extra_flags) if a.child == "fleet" else 0, c.byref(h)) == 0
    assert lib.adsb_set_format_scale(h, FMT_CU8, 2.0 / 255.0) == 0
    assert lib.adsb_streams_open(h, K) == 0
    hd = vp()
    if a.child == "pdus":
        lib.adsb_decode_pdus.argtypes = [vp, vp, vp, i32, vp]
        assert lib.adsb_create(FS, THR, 0, FLAG_TABLE | FLAG_DECODE, c.byref(hd)) == 0
    if a.child == "fleet":
        lib.adsb_stream_decoder_stats.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    # a pool of 2^26 samples: stream i's call k reads samples [(i * CALLS + k) * NS, + NS) of it (modulo the pool)
    dev = torch.device("cuda:0")
    POOL, blk = 1 << 26, 1 << 24
    fc = torch.cat([M.synth_iq_torch(blk, FS, 1000.0, 100 + b, dev) for b in range(POOL // blk)])
    u8 = torch.clamp(torch.floor(fc * 63.75 + 128.0), 0, 255).to(torch.uint8).contiguous()
    del fc
    torch.cuda.synchronize()
    host = u8.cpu().numpy().reshape(-1)                       # pageable
    bases = {"device": u8.data_ptr(), "host": host.ctypes.data}
    dt = np.dtype([("data", "<u8"), ("n", "<i8"), ("stream", "<i4"), ("flags", "<u4"), ("threshold", "<f4"), ("reserved", "<u4")])
    rec = np.dtype([("offset", "<i8"), ("peak", "<f4"), ("median", "<f4"), ("bits", "u1", (14,)), ("flags", "<u2")])
    out = np.empty(1 << 18, dtype=rec)
    first = np.zeros(K + 1, dtype=np.int32)
    n_out, n_fb = i32(0), i32(0)

    def tables(base):
        tabs = []
        for k in range(CALLS):
            t = np.zeros(K, dtype=dt)
            start = ((np.arange(K, dtype=np.int64) * CALLS + k) * NS) % POOL
            t["data"] = base + 2 * start
            t["n"], t["threshold"], t["stream"] = NS, THR, np.arange(K)
            tabs.append(t)
        return tabs

    res = {"what": a.child, "lib": a.lib, "box": torch.cuda.get_device_name(0)}
    rows = np.zeros(4096, dtype=np.dtype([("r", "u1", (72,))]))
    for where, fn in zip(("device", "host"), names):
        if a.child == "pdus" and where == "host":
            break
        f = getattr(lib, fn)
        tabs = tables(bases[where])
        times, recs = [], 0
        for rep in range(3):                                   # the first sequence warms up (buffers grow), two are timed
            for i in range(K):
                lib.adsb_stream_reset(h, i)
            for k in range(CALLS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = f(h, FMT_CU8, vp(tabs[k].ctypes.data), K, vp(out.ctypes.data), len(out), vp(first.ctypes.data),
                       c.byref(n_out), c.byref(n_fb))
                dtm = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and n_fb.value == 0, (rc, n_fb.value)
                if a.child == "pdus":
                    if rep != 1:
                        continue
                    # the call's records, stream by stream: the PDUs (BURST_DEMOD) and their timestamps
                    parts = []
                    for i in range(K):
                        r = out[first[i]:first[i + 1]]
                        r = r[(r["flags"] & 1) != 0]
                        if len(r):
                            parts.append((np.ascontiguousarray(r["bits"]), r["offset"].astype(np.float64) / FS))
                    t0 = time.perf_counter()
                    assert all(len(p[0]) <= len(rows) for p in parts)
                    for b, ts in parts:
                        assert lib.adsb_decode_pdus(hd, vp(b.ctypes.data), vp(ts.ctypes.data), len(b), vp(rows.ctypes.data)) == 0
                    dtm = (time.perf_counter() - t0) * 1e3
                    times.append(dtm)
                    recs += sum(len(p[0]) for p in parts)
                elif rep > 0:
                    times.append(dtm)
                    recs += n_out.value
        res[where] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                      "records": recs}
    if a.child == "fleet":
        p, cp, g = i64(0), i64(0), i64(0)
        assert lib.adsb_stream_decoder_stats(h, c.byref(p), c.byref(cp), c.byref(g)) == 0
        res["store"] = {"planes": p.value, "capacity": cp.value, "grows": g.value}
    if hd:
        lib.adsb_destroy(hd)
    lib.adsb_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    import numpy as np
    here = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    A, B, D_ = "(a) this build, flag", "(b) this build, no flag", "(d) adsb_decode_pdus per stream"
    C1, C2 = "(c) parent build, run 1", "(c) parent build, run 2"
    sides = [(A, here, "fleet"), (B, here, "stream"), (D_, here, "pdus")]
    if a.parent_lib:
        sides = [(C1, a.parent_lib, "stream")] + sides + [(C2, a.parent_lib, "stream")]
    say("%d streams x 2^%d-sample uint8 IQ chunks, 2 Msps, %d consecutive calls; median wall ms per call (two timed "
        "sequences per process; (d): one), %d rounds of fresh processes, the sides alternated" % (K, a.log2n, CALLS, a.rounds))
    box = None
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
            if box is None:
                box = res["box"]
                say("box: %s" % box)
            txt = "round %d  %-32s" % (r, name)
            for where in ("device", "host"):
                if where in res:
                    med[name][where].append(res[where]["median_ms"])
                    txt += "  %s %8.3f ms (min %.3f max %.3f, %d records)" % (where, res[where]["median_ms"], res[where]["min_ms"],
                                                                            res[where]["max_ms"], res[where]["records"])
            if "store" in res:
                txt += "  store: %(planes)d planes, %(capacity)d slots, %(grows)d growths" % res["store"]
            say(txt)
    say("")
    mid = {}
    for name, _, _ in sides:
        for where in ("device", "host"):
            v = med[name][where]
            if v:
                mid[name, where] = float(np.median(v))
                say("%-32s %-6s median of rounds %8.3f ms per call (%s)" % (name, where, mid[name, where], " ".join("%.3f" % t for t in v)))
    say("")
    for where in ("device", "host"):
        fa, fb = mid[A, where], mid[B, where]
        say("%-6s entry point: (a) / (b) = %.3f  (%.3f ms against %.3f ms per call: the decode step adds %.3f ms)" % (
            where, fa / fb, fa, fb, fa - fb))
        if a.parent_lib:
            c1, c2 = mid[C1, where], mid[C2, where]
            pc = 0.5 * (c1 + c2)
            tol = max(abs(x - y) for x, y in zip(med[C1][where], med[C2][where])) / pc
            tol = max(tol, abs(c1 - c2) / pc)
            d = abs(fb - pc) / pc
            say("%-6s entry point: (c) %.3f and %.3f ms (its two runs differ by up to %.1f %% within a round), (b) %.3f ms: %.1f %% from "
                "their mean -> %s" % (where, c1, c2, 100 * tol, fb, 100 * d,
                                      "agree within the spread" if d <= tol else "DIFFER by more than the spread"))
    dd = mid[D_, "device"]
    say("(d) %.3f ms per call's records; (d) / ((a) - (b)), device entry point = %.1f" % (dd, dd / (mid[A, "device"] - mid[B, "device"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
