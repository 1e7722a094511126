"""Cost of adsb_stream_mlat_rule, by the method of tools/mlat_cost.py and on its two carries: 1024 streams x 2^16-sample uint8 IQ
chunks at 2 Msps, 16 consecutive calls through the device entry point of an ADSB_FLAG_STREAM_DECODE | _SHARED | _DEDUP context
fill the carry; the receivers of a group stand on a 100 km circle and start at |p - R| / C for one aircraft position p.  Every
side is a fresh child process under a time limit of its own, the sides alternated, three rounds; the first non-zero exit ends
the run.
  (a) 16 groups of 64 receivers, (b) 128 groups of 8: one call over the full carry of
        gn      adsb_stream_mlat (the undamped rule),
        damped  adsb_stream_mlat_rule, ADSB_MLAT_SOLVER_LM | ADSB_MLAT_RESTART,
        aided   the same with ADSB_MLAT_ALTITUDE (alt_weight 1, min_rx 3): the replies that announce an altitude take the row;
      all on THIS build, aux rows downloaded.
  (p) adsb_stream_mlat on carry (a) and the shared + de-duplicating stream-batch step on this build against the PARENT commit's
      build (--parent-lib), which is run twice per round: the spread this build is held against.
No figure is fixed; (p) states whether this build lies within the parent's own run-to-run spread.
    python tools/mlat_rule_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 3] [--out profiles/mlat_rule_cost.txt]
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
ap.add_argument("--child", choices=["step", "gn", "damped", "aided"], default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--group", type=int, default=64)            # receivers that read the same samples
ap.add_argument("--child-timeout", type=int, default=300)
a = ap.parse_args()

FMT_CU8, FS, THR = 4, 2e6, 0.01
SD, SH, DD = 1024, 4096, 8192
K, NS, CALLS = a.streams, 1 << a.log2n, a.calls
C = 299702547.0
FIX = [("ts", "<f8"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("t_tx", "<f8"), ("rms_m", "<f8"), ("bits", "u1", (14,)), ("flags", "<u2"),
       ("icao", "<i4"), ("n_rx", "<i4"), ("n_heard", "<i4"), ("status", "<i4"), ("iters", "<i4"), ("first", "<i4")]
AUX = [("up_m", "<f8"), ("lambda", "<f8"), ("alt_ft", "<i4"), ("tries", "<i4"), ("flags", "<u4"), ("reserved", "<i4")]


class Rule(ctypes.Structure):
    _fields_ = [("solver", ctypes.c_int32), ("flags", ctypes.c_int32), ("min_rx", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("alt_weight", ctypes.c_double)]


def child():
    """one process, one library -> one JSON line: median wall ms per stream-batch call (step), or of the stated call over the
    carry those calls leave"""
    import numpy as np
    import torch
    from gr_adsb_amd import modulator as M
    c = ctypes
    lib = c.CDLL(a.lib)
    vp, i32, i64, f64 = c.c_void_p, c.c_int32, c.c_int64, c.c_double
    lib.adsb_create.argtypes = [f64, c.c_float, c.c_int, c.c_uint32, c.POINTER(vp)]
    lib.adsb_destroy.argtypes = [vp]
    lib.adsb_destroy.restype = None
    lib.adsb_set_format_scale.argtypes = [vp, c.c_int, c.c_float]
    lib.adsb_process_stream_batch_device.argtypes = [vp, c.c_int, vp, i32, vp, i32, vp, c.POINTER(i32), c.POINTER(i32)]
    lib.adsb_streams_open.argtypes = [vp, i32]
    lib.adsb_stream_reset.argtypes = [vp, i32]
    lib.adsb_streams_decoder_reset.argtypes = [vp]
    lib.adsb_stream_set_start.argtypes = [vp, i32, f64]
    lib.adsb_stream_dedup_stats.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(f64)]
    h = vp()
    assert lib.adsb_create(FS, THR, 0, SD | SH | DD, c.byref(h)) == 0
    assert lib.adsb_set_format_scale(h, FMT_CU8, 2.0 / 255.0) == 0
    assert lib.adsb_streams_open(h, K) == 0
    k_in = np.arange(K) % a.group
    ang = 2 * np.pi * k_in / a.group
    rx = np.stack([4.0e6 + 1.0e5 * np.cos(ang) - 800.0 * (k_in % 3), 1.0e5 * np.sin(ang), 5.0e6 + 1200.0 * (k_in % 2)], axis=1)
    p = np.array([4.0e6 + 7000.0, 12000.0, 5.0e6 + 9000.0])
    starts = np.sqrt(((rx - p) ** 2).sum(axis=1)) / C
    for s in range(K):
        assert lib.adsb_stream_set_start(h, s, float(starts[s])) == 0
    if a.child != "step":
        lib.adsb_stream_set_ecef.argtypes = [vp, i32, f64, f64, f64]
        lib.adsb_stream_mlat.argtypes = [vp, f64, f64, i32, vp, i32, c.POINTER(i32), vp, vp, i32, c.POINTER(i32)]
        if a.child != "gn":
            lib.adsb_stream_mlat_rule.argtypes = [vp, f64, f64, c.POINTER(Rule), vp, vp, i32, c.POINTER(i32), vp, vp, i32, c.POINTER(i32)]
        for s in range(K):
            assert lib.adsb_stream_set_ecef(h, s, *[float(v) for v in rx[s]]) == 0
    dev = torch.device("cuda:0")
    POOL, blk = 1 << 26, 1 << 24
    fc = torch.cat([M.synth_iq_torch(blk, FS, 1000.0, 100 + b, dev) for b in range(POOL // blk)])
    u8 = torch.clamp(torch.floor(fc * 63.75 + 128.0), 0, 255).to(torch.uint8).contiguous()
    del fc
    u8 = torch.cat([u8, u8[:2 * (NS + 8192 * 64)]]).contiguous()
    torch.cuda.synchronize()
    dt = np.dtype([("data", "<u8"), ("n", "<i8"), ("stream", "<i4"), ("flags", "<u4"), ("threshold", "<f4"), ("reserved", "<u4")])
    rec = np.dtype([("offset", "<i8"), ("peak", "<f4"), ("median", "<f4"), ("bits", "u1", (14,)), ("flags", "<u2")])
    out = np.empty(1 << 18, dtype=rec)
    first = np.zeros(K + 1, dtype=np.int32)
    n_out, n_fb = i32(0), i32(0)
    tabs = []
    for k in range(CALLS):                                    # tools/dedup_cost.py's tables
        t = np.zeros(K, dtype=dt)
        chunk = (np.arange(K, dtype=np.int64) // a.group) * CALLS + k
        t["data"] = u8.data_ptr() + 2 * ((chunk * NS) % POOL + 8192 * (chunk * NS // POOL))
        t["n"], t["threshold"], t["stream"] = NS, THR, np.arange(K)
        tabs.append(t)
    res = {"what": a.child, "lib": a.lib, "box": torch.cuda.get_device_name(0), "group": a.group}
    times = []
    for rep in range(3 if a.child == "step" else 1):           # step: the first sequence warms up, two are timed
        for i in range(K):
            lib.adsb_stream_reset(h, i)
        assert lib.adsb_streams_decoder_reset(h) == 0
        for k in range(CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.adsb_process_stream_batch_device(h, FMT_CU8, vp(tabs[k].ctypes.data), K, vp(out.ctypes.data), len(out), vp(first.ctypes.data),
                                                      c.byref(n_out), c.byref(n_fb))
            dtm = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and n_fb.value == 0, (rc, n_fb.value)
            if rep > 0:
                times.append(dtm)
    d, cr, hi = i64(0), i64(0), f64(0)
    assert lib.adsb_stream_dedup_stats(h, c.byref(d), c.byref(cr), c.byref(hi)) == 0
    res["duplicates"], res["carried"] = d.value, cr.value
    if a.child == "step":
        res["call"] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}
    else:
        rule = Rule(1, 1 | (2 if a.child == "aided" else 0), 3 if a.child == "aided" else 4, 0, 1.0)
        n, m = i32(0), i32(0)

        def call(fixes, aux, cap, ms, mt, member_cap):
            if a.child == "gn":
                return lib.adsb_stream_mlat(h, -np.inf, np.inf, 4, fixes, cap, c.byref(n), ms, mt, member_cap, c.byref(m))
            return lib.adsb_stream_mlat_rule(h, -np.inf, np.inf, c.byref(rule), fixes, aux, cap, c.byref(n), ms, mt, member_cap, c.byref(m))

        assert call(None, None, 0, None, None, 0) in (0, -28)
        fixes, aux = np.zeros(max(n.value, 1), dtype=np.dtype(FIX)), np.zeros(max(n.value, 1), dtype=np.dtype(AUX))
        ms, mt = np.zeros(max(m.value, 1), np.int32), np.zeros(max(m.value, 1), np.float64)
        times = []
        for rep in range(12):                                  # two warm up, ten are timed
            t0 = time.perf_counter()
            rc = call(vp(fixes.ctypes.data), vp(aux.ctypes.data), len(fixes), vp(ms.ctypes.data), vp(mt.ctypes.data), len(ms))
            dtm = (time.perf_counter() - t0) * 1e3
            assert rc == 0, rc
            if rep >= 2:
                times.append(dtm)
        fx, ax = fixes[:n.value], aux[:n.value]
        err = np.sqrt((fx["x"] - p[0]) ** 2 + (fx["y"] - p[1]) ** 2 + (fx["z"] - p[2]) ** 2) if len(fx) else np.zeros(0)
        res["call"] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)), "fixes": int(n.value),
                       "members": int(m.value), "ok": int((fx["status"] == 0).sum()), "mean_iters": float(fx["iters"].mean()) if len(fx) else 0.0,
                       "mean_n_rx": float(fx["n_rx"].mean()) if len(fx) else 0.0, "within_1m": int(((fx["status"] == 0) & (err < 1.0)).sum()),
                       "mean_tries": float(ax["tries"].mean()) if len(fx) and a.child != "gn" else 0.0,
                       "aided": int((ax["flags"] & 1).astype(bool).sum()) if a.child != "gn" else 0,
                       "restarted": int((ax["flags"] & 2).astype(bool).sum()) if a.child != "gn" else 0}
    lib.adsb_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    import numpy as np
    here = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sides = [("(%s) %s, %s" % (tag, what, desc), here, what, group)
             for tag, desc, group in (("a", "16 groups of 64", 64), ("b", "128 groups of 8", 8)) for what in ("gn", "damped", "aided")]
    GN_A, STEP = sides[0][0], "(p) this build, shared + dedup step"
    sides.append((STEP, here, "step", 64))
    P1, P2, M1, M2 = "(p) parent build, step, run 1", "(p) parent build, step, run 2", "(p) parent build, gn (a), run 1", "(p) parent build, gn (a), run 2"
    if a.parent_lib:
        sides = [(P1, a.parent_lib, "step", 64), (M1, a.parent_lib, "gn", 64)] + sides + [(P2, a.parent_lib, "step", 64), (M2, a.parent_lib, "gn", 64)]
    say("%d streams x 2^%d-sample uint8 IQ chunks, 2 Msps, %d consecutive calls fill the carry; one call over all of it: median wall ms "
        "of ten calls, downloads included; the step: median wall ms per call of two timed sequences; %d rounds of fresh processes, the "
        "sides alternated; window 2 ms, horizon 1 s" % (K, a.log2n, CALLS, a.rounds))
    med = {s[0]: [] for s in sides}
    last = {}
    box = None
    for r in range(a.rounds):
        for name, lib, what, group in sides:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", what, "--lib", lib,
                   "--group", str(group), "--streams", str(K), "--log2n", str(a.log2n), "--calls", str(CALLS)]
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
            v = res["call"]
            med[name].append(v["median_ms"])
            last[name] = res
            txt = "round %d  %-38s %8.3f ms (min %.3f max %.3f), carried %d" % (r, name, v["median_ms"], v["min_ms"], v["max_ms"], res["carried"])
            if what != "step":
                txt += "; %d fixes (%d OK, %d within 1 m of the aircraft, %.1f hearings, %.1f steps and %.1f trials each, %d aided, %d restarted), " \
                       "%d members" % (v["fixes"], v["ok"], v["within_1m"], v["mean_n_rx"], v["mean_iters"], v["mean_tries"], v["aided"], v["restarted"],
                                       v["members"])
            say(txt)
            if a.out:                                         # what is measured so far survives a later side's failure
                open(a.out, "w").write("\n".join(lines) + "\n")
    say("")
    mid = {}
    for name, _, _, _ in sides:
        mid[name] = float(np.median(med[name]))
        say("%-38s median of rounds %8.3f ms (%s)" % (name, mid[name], " ".join("%.3f" % t for t in med[name])))
    say("")
    for k in (0, 3):
        gn = sides[(2 if a.parent_lib else 0) + k][0]
        for j in (1, 2):
            name = sides[(2 if a.parent_lib else 0) + k + j][0]
            say("%s: %.3f ms against %.3f ms of adsb_stream_mlat on the same carry (%.2fx)" % (name, mid[name], mid[gn], mid[name] / mid[gn]))
    if a.parent_lib:
        for what, this, p1, p2 in (("the step", STEP, P1, P2), ("adsb_stream_mlat (a)", GN_A, M1, M2)):
            c1, c2 = mid[p1], mid[p2]
            pc = 0.5 * (c1 + c2)
            tol = max(max(abs(x - y) for x, y in zip(med[p1], med[p2])), abs(c1 - c2)) / pc
            dd = abs(mid[this] - pc) / pc
            say("(p) %s: parent %.3f and %.3f ms (its two runs differ by up to %.1f %% within a round), this build %.3f ms: %.1f %% from their "
                "mean -> %s" % (what, c1, c2, 100 * tol, mid[this], 100 * dd, "agree within the spread" if dd <= tol else "DIFFER by more than the spread"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
