"""Cost of ADSB_FLAG_STREAM_DEDUP on the workload and by the method of tools/shared_decode_cost.py: 1024 streams x 2^16-sample
uint8 IQ chunks at 2 Msps, 16 consecutive calls, median wall ms per call (a call ends in a stream synchronise), device and
host entry point, every side a fresh child process under a time limit of its own, the sides alternated, three rounds; the
first non-zero exit ends the run.  All streams start at 0, so a record's timestamp is offset / fs.
  (1) random payloads: the flag on against ADSB_FLAG_STREAM_DECODE_SHARED alone on this build.  Every stream reads its own
      samples (streams that share a chunk of the pool read it 4 ms apart), so nothing is a duplicate: the pure cost of the step;
  (2) the same with the fleet in 16 groups of 64 receivers that read the same samples: 63 of 64 hearings are duplicates, the
      decode step shrinks 64-fold and the scan grows;
  (3) the host alternative for (2): a context without a decoder, the call's records de-duplicated with a Python dict (payload
      -> last hearing) and the rest decoded with adsb_decode_pdus on an ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE context;
      the time is that of the dict and the decode calls, without the stream-batch call itself;
  (4) the flag-off shared step on this build against the PARENT commit's build (--parent-lib: its libadsb_hip.so), which is
      run twice per round: the spread the flag-off path is held against.
No ratio is fixed for (1) to (3); (4) states whether the flag-off path lies within the parent's own run-to-run spread.
    python tools/dedup_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 3] [--out profiles/dedup_cost.txt]
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
ap.add_argument("--child", choices=["fleet", "host"], default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--flags", type=int, default=0)
ap.add_argument("--group", type=int, default=1)             # receivers that read the same samples
ap.add_argument("--child-timeout", type=int, default=300)
a = ap.parse_args()

FMT_CU8, FS, THR = 4, 2e6, 0.01
FLAG_TABLE, FLAG_DECODE, SD, SH, DD = 256, 512, 1024, 4096, 8192
K, NS, CALLS = a.streams, 1 << a.log2n, a.calls
WINDOW = 0.002


def child():
    """one process, one library -> one JSON line: median wall ms per call of the device and the host entry point (fleet), or
    of the host's own de-duplication and decoding of a call's records (host)"""
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
    lib.adsb_streams_decoder_reset.argtypes = [vp]
    h = vp()
    assert lib.adsb_create(FS, THR, 0, a.flags, c.byref(h)) == 0
    assert lib.adsb_set_format_scale(h, FMT_CU8, 2.0 / 255.0) == 0
    assert lib.adsb_streams_open(h, K) == 0
    hd = vp()
    if a.child == "host":
        lib.adsb_decode_pdus.argtypes = [vp, vp, vp, i32, vp]
        assert lib.adsb_create(FS, THR, 0, FLAG_TABLE | FLAG_DECODE, c.byref(hd)) == 0
    if a.flags & DD:
        lib.adsb_stream_dedup_stats.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(c.c_double)]
    # a pool of 2^26 samples, 1024 chunks: group g's call k reads chunk g * CALLS + k (modulo the pool); groups that come to
    # share a chunk read it 8192 samples (4 ms) apart, which no window of 2 ms joins
    dev = torch.device("cuda:0")
    POOL, blk = 1 << 26, 1 << 24
    fc = torch.cat([M.synth_iq_torch(blk, FS, 1000.0, 100 + b, dev) for b in range(POOL // blk)])
    u8 = torch.clamp(torch.floor(fc * 63.75 + 128.0), 0, 255).to(torch.uint8).contiguous()
    del fc
    u8 = torch.cat([u8, u8[:2 * (NS + 8192 * 64)]]).contiguous()      # (a shifted chunk may run past the pool's end)
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
            g = np.arange(K, dtype=np.int64) // a.group
            chunk = g * CALLS + k
            start = (chunk * NS) % POOL + 8192 * (chunk * NS // POOL)
            t["data"] = base + 2 * start
            t["n"], t["threshold"], t["stream"] = NS, THR, np.arange(K)
            tabs.append(t)
        return tabs

    res = {"what": a.child, "lib": a.lib, "box": torch.cuda.get_device_name(0), "duplicates": 0, "carried": 0}
    rows = np.zeros(4096, dtype=np.dtype([("r", "u1", (72,))]))
    for where, fn in zip(("device", "host"), names):
        if a.child == "host" and where == "host":
            break
        f = getattr(lib, fn)
        tabs = tables(bases[where])
        times, recs = [], 0
        for rep in range(3):                                   # the first sequence warms up (buffers grow), two are timed
            for i in range(K):
                lib.adsb_stream_reset(h, i)
            if a.flags & SH:
                assert lib.adsb_streams_decoder_reset(h) == 0  # a fresh decoder, an empty carry: every sequence is the same work
            for k in range(CALLS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = f(h, FMT_CU8, vp(tabs[k].ctypes.data), K, vp(out.ctypes.data), len(out), vp(first.ctypes.data),
                       c.byref(n_out), c.byref(n_fb))
                dtm = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and n_fb.value == 0, (rc, n_fb.value)
                if a.child == "host":
                    if rep != 1:
                        continue
                    r = out[:n_out.value].copy()
                    stream = np.repeat(np.arange(K), np.diff(first))
                    t0 = time.perf_counter()
                    dem = (r["flags"] & 1) != 0
                    r, stream = r[dem], stream[dem]
                    ts = r["offset"].astype(np.float64) / FS
                    order = np.argsort(ts, kind="stable")
                    lng = (r["flags"] & 64) != 0
                    seen, keep = {}, []
                    for t in order.tolist():
                        key = r["bits"][t].tobytes() if lng[t] else r["bits"][t][:7].tobytes()
                        q = seen.get(key)
                        if q is None or q[1] == stream[t] or abs(ts[t] - q[0]) > WINDOW:
                            keep.append(t)
                        seen[key] = (ts[t], stream[t])
                    b, tk = np.ascontiguousarray(r["bits"][keep]), np.ascontiguousarray(ts[keep])
                    for lo in range(0, len(b), len(rows)):
                        n = min(len(rows), len(b) - lo)
                        assert lib.adsb_decode_pdus(hd, vp(b[lo:].ctypes.data), vp(tk[lo:].ctypes.data), n, vp(rows.ctypes.data)) == 0
                    dtm = (time.perf_counter() - t0) * 1e3
                    times.append(dtm)
                    recs += len(keep)
                elif rep > 0:
                    times.append(dtm)
                    recs += n_out.value
            if a.flags & DD:
                d, cr, hi = i64(0), i64(0), c.c_double(0)
                assert lib.adsb_stream_dedup_stats(h, c.byref(d), c.byref(cr), c.byref(hi)) == 0
                res["duplicates"], res["carried"] = d.value, cr.value
        res[where] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                      "records": recs}
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

    ON1, OFF1 = "(1) dedup, random payloads", "(1)/(4) shared alone, random payloads"
    ON2, OFF2, HOST = "(2) dedup, 16 groups of 64", "(2) shared alone, 16 groups of 64", "(3) host dict + adsb_decode_pdus, 16 x 64"
    P1, P2 = "(4) parent build, shared, run 1", "(4) parent build, shared, run 2"
    sides = [(ON1, here, "fleet", SD | SH | DD, 1), (OFF1, here, "fleet", SD | SH, 1), (ON2, here, "fleet", SD | SH | DD, 64),
             (OFF2, here, "fleet", SD | SH, 64), (HOST, here, "host", 0, 64)]
    if a.parent_lib:
        sides = [(P1, a.parent_lib, "fleet", SD | SH, 1)] + sides + [(P2, a.parent_lib, "fleet", SD | SH, 1)]
    say("%d streams x 2^%d-sample uint8 IQ chunks, 2 Msps, %d consecutive calls; median wall ms per call (two timed sequences "
        "per process; (3): one), %d rounds of fresh processes, the sides alternated; window 2 ms, horizon 1 s (the defaults)"
        % (K, a.log2n, CALLS, a.rounds))
    say("kernel launches of the decode step per call: shared 54; with the flag 58 (+ k_dedup_entries, k_dedup_find, k_dedup_merge, "
        "k_dedup_mark), one more upload (the items' streams) and one more download (dup[])")
    box = None
    med = {s[0]: {"device": [], "host": []} for s in sides}
    for r in range(a.rounds):
        for name, lib, what, flags, group in sides:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", what, "--lib", lib,
                   "--flags", str(flags), "--group", str(group), "--streams", str(K), "--log2n", str(a.log2n), "--calls", str(CALLS)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                say("round %d, %s: exit %d -- stopping\n%s" % (r, name, p.returncode, p.stdout[-2000:]))
                if a.out:
                    open(a.out, "w").write("\n".join(lines) + "\n")
                return p.returncode
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            if box is None:
                box = res["box"]
                say("box: %s" % box)
            txt = "round %d  %-42s" % (r, name)
            for where in ("device", "host"):
                if where in res:
                    med[name][where].append(res[where]["median_ms"])
                    txt += "  %s %8.3f ms (min %.3f max %.3f, %d records)" % (where, res[where]["median_ms"], res[where]["min_ms"],
                                                                            res[where]["max_ms"], res[where]["records"])
            if flags & DD:
                txt += "  duplicates %d, carried %d" % (res["duplicates"], res["carried"])
            say(txt)
    say("")
    mid = {}
    for name, _, _, _, _ in sides:
        for where in ("device", "host"):
            v = med[name][where]
            if v:
                mid[name, where] = float(np.median(v))
                say("%-42s %-6s median of rounds %8.3f ms per call (%s)" % (name, where, mid[name, where], " ".join("%.3f" % t for t in v)))
    say("")
    for where in ("device", "host"):
        for tag, on, off in (("(1)", ON1, OFF1), ("(2)", ON2, OFF2)):
            fa, fb = mid[on, where], mid[off, where]
            say("%s %-6s entry point: flag on / shared alone = %.3f  (%.3f ms against %.3f ms per call: %+.3f ms)" % (
                tag, where, fa / fb, fa, fb, fa - fb))
        if a.parent_lib:
            fb = mid[OFF1, where]
            c1, c2 = mid[P1, where], mid[P2, where]
            pc = 0.5 * (c1 + c2)
            tol = max(abs(x - y) for x, y in zip(med[P1][where], med[P2][where])) / pc
            tol = max(tol, abs(c1 - c2) / pc)
            d = abs(fb - pc) / pc
            say("(4) %-6s entry point: parent %.3f and %.3f ms (its two runs differ by up to %.1f %% within a round), this build, flag off "
                "%.3f ms: %.1f %% from their mean -> %s" % (where, c1, c2, 100 * tol, fb, 100 * d,
                                                           "agree within the spread" if d <= tol else "DIFFER by more than the spread"))
    hd = mid[HOST, "device"]
    say("(3) the host's dict and adsb_decode_pdus: %.3f ms per call's records, against %+.3f ms for the flag in (2) (device entry point)"
        % (hd, mid[ON2, "device"] - mid[OFF2, "device"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
