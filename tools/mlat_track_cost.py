"""Cost of the MLAT track store, by the method of tools/mlat_rule_cost.py and on its two carries: 1024 streams x 2^16-sample uint8 IQ
chunks at 2 Msps, 16 consecutive calls through the device entry point of an ADSB_FLAG_STREAM_DECODE | _SHARED | _DEDUP context
fill the carry (474 304 hearings); the receivers of a group stand on a 100 km circle and start at |p - R| / C for one aircraft
position p.  Every side is a fresh child process under a time limit of its own, the sides alternated, three rounds; the first
non-zero exit ends the run.
  (a) 16 groups of 64 receivers, (b) 128 groups of 8, (w) 128 groups of 8 whose every reply is a DF 17 of one of 24 addresses -- the
      worst case: every fix eligible, 24 runs, one lane walking each:
        rule    one adsb_stream_mlat_rule call (ADSB_MLAT_SOLVER_LM | ADSB_MLAT_RESTART) over the full carry, downloads included:
                the yardstick, an existing call whose kernels this change does not touch;
        track   one adsb_stream_mlat_track call with the same rule over the same carry into an EMPTY store (the store is reset
                before every timed call, so every call does the same work; nothing comes down but the counts); then three calls
                onto the store that leaves, each timed alone: every fix is stale, and the first is the first to move old rows.
      The replies of (a) and (b) carry random fields, so 9 of 32 are eligible and nearly every eligible fix starts a track of its
      own: the insertion-heavy case.
  (p) adsb_stream_mlat_rule on carry (a) and the shared + de-duplicating stream-batch step on this build against the PARENT
      commit's build (--parent-lib), which is run twice per round: the spread this build is held against.
  (s) once: readout (adsb_stream_mlat_tracks, everything) and expiry (adsb_stream_mlat_tracks_expire: none removed, and the older
      half removed) at about 10^3 and about 10^5 tracks, built from DF 17 replies of random addresses; the counts are stated.
No figure is fixed in advance.
    python tools/mlat_track_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 3] [--out profiles/mlat_track_cost.txt]
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
ap.add_argument("--child", choices=["step", "rule", "track", "store"], default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--group", type=int, default=64)            # receivers that read the same samples
ap.add_argument("--addresses", type=int, default=0)         # > 0: every reply a DF 17 of one of that many addresses; -1: of random ones
ap.add_argument("--child-timeout", type=int, default=300)
a = ap.parse_args()

FMT_CU8, FS, THR = 4, 2e6, 0.01
SD, SH, DD = 1024, 4096, 8192
K, NS, CALLS = a.streams, 1 << a.log2n, a.calls
C = 299702547.0
FIX = [("ts", "<f8"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("t_tx", "<f8"), ("rms_m", "<f8"), ("bits", "u1", (14,)), ("flags", "<u2"),
       ("icao", "<i4"), ("n_rx", "<i4"), ("n_heard", "<i4"), ("status", "<i4"), ("iters", "<i4"), ("first", "<i4")]
AUX = [("up_m", "<f8"), ("lambda", "<f8"), ("alt_ft", "<i4"), ("tries", "<i4"), ("flags", "<u4"), ("reserved", "<i4")]
STATS = ("fixes", "eligible", "unusable", "stale", "rejected", "taken", "started", "tracks")


class Rule(ctypes.Structure):
    _fields_ = [("solver", ctypes.c_int32), ("flags", ctypes.c_int32), ("min_rx", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("alt_weight", ctypes.c_double)]


class TrackRule(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("alpha", "beta", "gate_m", "max_speed_mps", "max_gap_s", "max_rms_m", "min_up_m")] + \
               [("restart_after", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def child():
    """one process, one library -> one JSON line"""
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
        lib.adsb_stream_mlat_rule.argtypes = [vp, f64, f64, c.POINTER(Rule), vp, vp, i32, c.POINTER(i32), vp, vp, i32, c.POINTER(i32)]
        for s in range(K):
            assert lib.adsb_stream_set_ecef(h, s, *[float(v) for v in rx[s]]) == 0
    if a.child in ("track", "store"):
        lib.adsb_stream_mlat_track.argtypes = [vp, f64, f64, c.POINTER(Rule), c.POINTER(TrackRule), vp]
        lib.adsb_stream_mlat_tracks.argtypes = [vp, i32, f64, vp, i32, c.POINTER(i32)]
        lib.adsb_stream_mlat_tracks_expire.argtypes = [vp, f64, c.POINTER(i64)]
        lib.adsb_stream_mlat_tracks_reset.argtypes = [vp]
    dev = torch.device("cuda:0")
    POOL, blk = (1 << 28) if a.child == "store" else (1 << 26), 1 << 24      # (store: room for 10^5 different replies)
    addresses = None
    if a.addresses > 0:
        addresses = [0x400000 + 4099 * k for k in range(a.addresses)]
    elif a.addresses < 0:
        addresses = np.random.default_rng(3).choice(1 << 24, 1 << 20, replace=False)
    fc = torch.cat([M.synth_iq_torch(blk, FS, 1000.0, 100 + b, dev, addresses=addresses) for b in range(POOL // blk)])
    u8 = torch.clamp(torch.floor(fc * 63.75 + 128.0), 0, 255).to(torch.uint8).contiguous()
    del fc
    u8 = torch.cat([u8, u8[:2 * (NS + 8192 * 64)]]).contiguous()
    torch.cuda.synchronize()
    dt = np.dtype([("data", "<u8"), ("n", "<i8"), ("stream", "<i4"), ("flags", "<u4"), ("threshold", "<f4"), ("reserved", "<u4")])
    rec = np.dtype([("offset", "<i8"), ("peak", "<f4"), ("median", "<f4"), ("bits", "u1", (14,)), ("flags", "<u2")])
    out = np.empty(1 << 18, dtype=rec)
    first = np.zeros(K + 1, dtype=np.int32)
    n_out, n_fb = i32(0), i32(0)

    def table(k):                                             # tools/dedup_cost.py's tables; k >= CALLS: the chunks behind the first fill's
        t = np.zeros(K, dtype=dt)
        chunk = (np.arange(K, dtype=np.int64) // a.group) * CALLS + k % CALLS + (k // CALLS) * (K // a.group) * CALLS
        t["data"] = u8.data_ptr() + 2 * ((chunk * NS) % POOL + 8192 * (chunk * NS // POOL))
        t["n"], t["threshold"], t["stream"] = NS, THR, np.arange(K)
        return t

    def fill(k0, timed=None):
        for i in range(K):
            lib.adsb_stream_reset(h, i)
        assert lib.adsb_streams_decoder_reset(h) == 0
        for k in range(k0, k0 + CALLS):
            t = table(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.adsb_process_stream_batch_device(h, FMT_CU8, vp(t.ctypes.data), K, vp(out.ctypes.data), len(out), vp(first.ctypes.data),
                                                      c.byref(n_out), c.byref(n_fb))
            dtm = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and n_fb.value == 0, (rc, n_fb.value)
            if timed is not None:
                timed.append(dtm)

    res = {"what": a.child, "lib": a.lib, "box": torch.cuda.get_device_name(0), "group": a.group}
    times = []
    for rep in range(3 if a.child == "step" else 1):           # step: the first sequence warms up, two are timed
        fill(0, times if rep > 0 else None)
    d, cr, hi = i64(0), i64(0), f64(0)
    assert lib.adsb_stream_dedup_stats(h, c.byref(d), c.byref(cr), c.byref(hi)) == 0
    res["duplicates"], res["carried"] = d.value, cr.value
    rule = Rule(1, 1, 4, 0, 1.0)
    trule = TrackRule(0.3, 0.05, 2000.0, 350.0, 30.0, 500.0, 0.0, 3, 0)
    st = (i64 * 8)()

    def track(t_lo=-np.inf, t_hi=np.inf):
        rc = lib.adsb_stream_mlat_track(h, t_lo, t_hi, c.byref(rule), c.byref(trule), st)
        assert rc == 0, rc
        return dict(zip(STATS, (int(v) for v in st)))

    def timed_ms(fn, reps=1):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps

    summary = lambda ts: {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}      # noqa: E731
    if a.child == "step":
        res["call"] = summary(times)
    elif a.child == "rule":
        n, m = i32(0), i32(0)

        def call(fixes, aux, cap, ms, mt, member_cap):
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
        fx = fixes[:n.value]
        res["call"] = dict(summary(times), fixes=int(n.value), eligible=int((fx["icao"] >= 0).sum()), addresses=int(len(np.unique(fx["icao"][fx["icao"] >= 0]))))
    elif a.child == "track":
        times = []
        for rep in range(12):                                  # two warm up, ten are timed; every call fills an empty store
            assert lib.adsb_stream_mlat_tracks_reset(h) == 0
            t0 = time.perf_counter()
            s = track()
            dtm = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                times.append(dtm)
        again_ms = []                                           # and three more onto the store it left: every fix stale.  The first of
        for rep in range(3):                                    # them is the process's first call with old rows to move
            t0 = time.perf_counter()
            again = track()
            again_ms.append((time.perf_counter() - t0) * 1e3)
        res["call"] = dict(summary(times), again_ms=again_ms, again_stale=again["stale"], **s)
    else:                                                       # store
        lo = float(starts.min())
        rows = np.zeros(1 << 18, dtype=np.dtype([("raw", "u1", (96,))]))
        n, removed = i32(0), i64(0)
        res["sizes"] = []
        for want in (1000, 100000):
            assert lib.adsb_stream_mlat_tracks_reset(h) == 0
            fill(0)
            s = track(-np.inf, lo + (hi.value - lo) * want / 59000.0) if want < 50000 else track()
            if want >= 50000:                                   # a second carry of other chunks of the pool: other addresses
                fill(CALLS)
                s = track()
            nt = s["tracks"]
            read = [timed_ms(lambda: lib.adsb_stream_mlat_tracks(h, 1, -np.inf, vp(rows.ctypes.data), len(rows), c.byref(n))) for _ in range(7)][2:]
            assert n.value == nt
            count = [timed_ms(lambda: lib.adsb_stream_mlat_tracks(h, 1, -np.inf, None, 0, c.byref(n))) for _ in range(7)][2:]
            none = [timed_ms(lambda: lib.adsb_stream_mlat_tracks_expire(h, -np.inf, c.byref(removed))) for _ in range(7)][2:]
            last = np.sort(rows[:nt]["raw"][:, 24:32].copy().view("<f8").reshape(-1))
            half = timed_ms(lambda: lib.adsb_stream_mlat_tracks_expire(h, float(last[nt // 2]), c.byref(removed)))
            res["sizes"].append({"tracks": nt, "readout_ms": float(np.median(read)), "count_query_ms": float(np.median(count)),
                                 "expire_none_ms": float(np.median(none)), "expire_half_ms": half, "half_removed": int(removed.value)})
    lib.adsb_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    import numpy as np
    here = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")

    carries = (("a", "16 groups of 64", 64, 0), ("b", "128 groups of 8", 8, 0), ("w", "128 groups of 8, 24 addresses", 8, 24))
    sides = [("(%s) %s, %s" % (tag, what, desc), here, what, group, addr) for tag, desc, group, addr in carries for what in ("rule", "track")]
    RULE_A, STEP = sides[0][0], "(p) this build, shared + dedup step"
    sides.append((STEP, here, "step", 64, 0))
    P1, P2, M1, M2 = "(p) parent build, step, run 1", "(p) parent build, step, run 2", "(p) parent build, rule (a), run 1", "(p) parent build, rule (a), run 2"
    if a.parent_lib:
        sides = [(P1, a.parent_lib, "step", 64, 0), (M1, a.parent_lib, "rule", 64, 0)] + sides + [(P2, a.parent_lib, "step", 64, 0), (M2, a.parent_lib, "rule", 64, 0)]
    say("%d streams x 2^%d-sample uint8 IQ chunks, 2 Msps, %d consecutive calls fill the carry; one call over all of it: median wall ms of ten "
        "calls, host clock around the blocking call; rule: adsb_stream_mlat_rule (damped, restart), downloads included; track: "
        "adsb_stream_mlat_track with the same rule into an empty store; the step: median wall ms per call of two timed sequences; %d rounds of "
        "fresh processes, the sides alternated; window 2 ms, horizon 1 s" % (K, a.log2n, CALLS, a.rounds))

    def run(name, lib, what, group, addr, r):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", what, "--lib", lib,
               "--group", str(group), "--addresses", str(addr), "--streams", str(K), "--log2n", str(a.log2n), "--calls", str(CALLS)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            say("round %s, %s: exit %d -- stopping\n%s" % (r, name, p.returncode, p.stdout[-2000:]))
            flush()
            return None
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    med = {s[0]: [] for s in sides}
    box = None
    for r in range(a.rounds):
        for name, lib, what, group, addr in sides:
            res = run(name, lib, what, group, addr, r)
            if res is None:
                return 1
            if box is None:
                box = res["box"]
                say("box: %s" % box)
            v = res["call"]
            med[name].append(v["median_ms"])
            txt = "round %d  %-44s %8.3f ms (min %.3f max %.3f), carried %d" % (r, name, v["median_ms"], v["min_ms"], v["max_ms"], res["carried"])
            if what == "rule":
                txt += "; %d fixes, %d eligible of %d addresses" % (v["fixes"], v["eligible"], v["addresses"])
            if what == "track":
                txt += "; %d fixes, %d eligible, %d unusable, %d started, %d taken, %d rejected, %d tracks; again onto that store %s ms (%d stale)" % (
                    v["fixes"], v["eligible"], v["unusable"], v["started"], v["taken"], v["rejected"], v["tracks"],
                    " / ".join("%.3f" % t for t in v["again_ms"]), v["again_stale"])
            say(txt)
            flush()                                           # what is measured so far survives a later side's failure
    say("")
    mid = {}
    for name, _, _, _, _ in sides:
        mid[name] = float(np.median(med[name]))
        say("%-44s median of rounds %8.3f ms (%s)" % (name, mid[name], " ".join("%.3f" % t for t in med[name])))
    say("")
    base = 2 if a.parent_lib else 0
    for k in (0, 2, 4):
        rule_name, track_name = sides[base + k][0], sides[base + k + 1][0]
        say("%s: %.3f ms against %.3f ms of adsb_stream_mlat_rule on the same carry (%.2fx)" % (track_name, mid[track_name], mid[rule_name],
                                                                                               mid[track_name] / mid[rule_name]))
    if a.parent_lib:
        for what, this, p1, p2 in (("the step", STEP, P1, P2), ("adsb_stream_mlat_rule (a)", RULE_A, M1, M2)):
            c1, c2 = mid[p1], mid[p2]
            pc = 0.5 * (c1 + c2)
            tol = max(max(abs(x - y) for x, y in zip(med[p1], med[p2])), abs(c1 - c2)) / pc
            dd = abs(mid[this] - pc) / pc
            say("(p) %s: parent %.3f and %.3f ms (its two runs differ by up to %.1f %% within a round), this build %.3f ms: %.1f %% from their "
                "mean -> %s" % (what, c1, c2, 100 * tol, mid[this], 100 * dd, "agree within the spread" if dd <= tol else "DIFFER by more than the spread"))
    flush()
    res = run("(s) readout and expiry", here, "store", 8, -1, "s")
    if res is None:
        return 1
    say("")
    for v in res["sizes"]:
        say("(s) %d tracks: readout of all %.3f ms, count query %.3f ms, expiry that removes none %.3f ms, expiry of the older half "
            "(%d removed) %.3f ms" % (v["tracks"], v["readout_ms"], v["count_query_ms"], v["expire_none_ms"], v["half_removed"], v["expire_half_ms"]))
    flush()
    return 0


if __name__ == "__main__":
    if a.child:
        child()
    else:
        sys.exit(main())
