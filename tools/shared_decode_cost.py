"""Cost of ONE decoder behind all receiver streams (ADSB_FLAG_STREAM_DECODE_SHARED) on the workload of
tools/stream_decode_cost.py: 1024 streams x 2^16-sample uint8 IQ chunks at 2 Msps, 16 consecutive calls.  The children are
that tool's own (its --child fleet with --extra-flags), each a fresh process under a time limit of its own; the first
non-zero exit ends the run.  Median wall ms per call, device and host entry point:
  (a) ADSB_FLAG_STREAM_DECODE | ADSB_FLAG_STREAM_DECODE_SHARED on this build: the time order (k_shared_keys, 24 sort launches,
      k_shared_gather), the decode step on one item, k_shared_scatter;
  (b) ADSB_FLAG_STREAM_DECODE alone on this build: one decoder per stream;
  (c) ADSB_FLAG_STREAM_DECODE alone on the PARENT commit's build (--parent-lib: its libadsb_hip.so), run TWICE per round, the
      sides alternated: the run-to-run spread that (b) is held against.
The file states (a) / (b) as measured -- no ratio is fixed for the shared step -- and whether (b) and (c) agree within the
spread of (c)'s two runs: the flag-off path must not have moved.
    python tools/shared_decode_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 3] [--out profiles/shared_decode_cost.txt]
(GPU box only.)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tools", "stream_decode_cost.py")
FLAG_SHARED = 4096

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--streams", type=int, default=1024)
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--calls", type=int, default=16)
ap.add_argument("--child-timeout", type=int, default=240)
a = ap.parse_args()


def main():
    here = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    A, B = "(a) this build, shared", "(b) this build, per stream"
    C1, C2 = "(c) parent build, per stream, run 1", "(c) parent build, per stream, run 2"
    sides = [(A, here, FLAG_SHARED), (B, here, 0)]
    if a.parent_lib:
        sides = [(C1, a.parent_lib, 0)] + sides + [(C2, a.parent_lib, 0)]
    say("%d streams x 2^%d-sample uint8 IQ chunks, 2 Msps, %d consecutive calls; median wall ms per call (two timed sequences "
        "per process), %d rounds of fresh processes, the sides alternated" % (a.streams, a.log2n, a.calls, a.rounds))
    say("kernel launches of the decode step per call: per stream 27 (5 table and classify, 21 key sort, 1 fold); shared 54 "
        "(+ k_shared_keys, 24 pair sort, k_shared_gather, k_shared_scatter) and one device-to-device copy of the timestamps")
    box = None
    med = {s[0]: {"device": [], "host": []} for s in sides}
    for r in range(a.rounds):
        for name, lib, extra in sides:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, CHILD, "--child", "fleet", "--lib", lib, "--extra-flags", str(extra),
                   "--streams", str(a.streams), "--log2n", str(a.log2n), "--calls", str(a.calls)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                say("round %d, %s: exit %d -- stopping\n%s" % (r, name, p.returncode, p.stdout[-2000:]))
                return p.returncode
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            if box is None:
                box = res["box"]
                say("box: %s" % box)
            txt = "round %d  %-38s" % (r, name)
            for where in ("device", "host"):
                med[name][where].append(res[where]["median_ms"])
                txt += "  %s %8.3f ms (min %.3f max %.3f, %d records)" % (where, res[where]["median_ms"], res[where]["min_ms"],
                                                                        res[where]["max_ms"], res[where]["records"])
            txt += "  store: %(planes)d planes, %(capacity)d slots, %(grows)d growths" % res["store"]
            say(txt)
    say("")
    mid = {}
    for name, _, _ in sides:
        for where in ("device", "host"):
            v = med[name][where]
            mid[name, where] = float(np.median(v))
            say("%-38s %-6s median of rounds %8.3f ms per call (%s)" % (name, where, mid[name, where], " ".join("%.3f" % t for t in v)))
    say("")
    for where in ("device", "host"):
        fa, fb = mid[A, where], mid[B, where]
        say("%-6s entry point: (a) / (b) = %.3f  (%.3f ms against %.3f ms per call: one shared decoder costs %+.3f ms more than one "
            "per stream)" % (where, fa / fb, fa, fb, fa - fb))
        if a.parent_lib:
            c1, c2 = mid[C1, where], mid[C2, where]
            pc = 0.5 * (c1 + c2)
            tol = max(abs(x - y) for x, y in zip(med[C1][where], med[C2][where])) / pc
            tol = max(tol, abs(c1 - c2) / pc)
            d = abs(fb - pc) / pc
            say("%-6s entry point: (c) %.3f and %.3f ms (its two runs differ by up to %.1f %% within a round), (b) %.3f ms: %.1f %% from "
                "their mean -> %s" % (where, c1, c2, 100 * tol, fb, 100 * d,
                                      "agree within the spread" if d <= tol else "DIFFER by more than the spread"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
