"""Cost of the plane ages (ADSB_FLAG_PLANE_AGES): what the flag costs the decode step, and what an expiry costs.
  (a) the decode step with the flag OFF: the workload of tools/stream_decode_cost.py (1024 streams x 2^16-sample uint8 chunks,
      ADSB_FLAG_STREAM_DECODE, median wall ms per call, fresh child processes) on this build against the PARENT commit's build
      (--parent-lib), the parent run twice per round: its run-to-run spread is what the difference is held against;
  (b) the same with the flag ON, as it comes;
  (c) one adsb_planes_expire on a decoder holding 10^3 and 10^5 planes, removing none and removing all, beside the time one
      read of the scanned 128 MiB takes at the read-only ceiling of DESIGN.md section 6;
  (d) one adsb_stream_planes_expire on stores of 65536 and 2^20 slots (1024 streams, 24 planes each), removing none and
      removing all, beside one read of the store.  The parent's ordinary rehash has no entry point of its own (it runs inside
      a stream-batch call), so it is not timed here.
(c) and (d): host clock around the blocking call, median (min .. max) of --reps calls.
    python tools/expire_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 2] [--out profiles/plane_expire_cost.txt]
(GPU box only.)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=None)
ap.add_argument("--child-timeout", type=int, default=200)
a = ap.parse_args()
lines = []
CEILING = (0.843 * 8e12, 0.874 * 8e12)        # bytes / s


def say(s):
    print(s, flush=True)
    lines.append(s)


def scale(nbytes):
    return "%.1f-%.1f" % (nbytes / CEILING[1] * 1e6, nbytes / CEILING[0] * 1e6)


def decode_step():
    here = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    P1, OFF, ON, P2 = "parent build, run 1", "(a) this build, flag off", "(b) this build, flag on", "parent build, run 2"
    sides = [(OFF, here, 0), (ON, here, 2048)]
    if a.parent_lib:
        sides = [(P1, a.parent_lib, 0)] + sides + [(P2, a.parent_lib, 0)]
    med = {s[0]: {"device": [], "host": []} for s in sides}
    tool = os.path.join(ROOT, "tools", "stream_decode_cost.py")
    for r in range(a.rounds):
        for name, lib, extra in sides:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, tool, "--child", "fleet", "--lib", lib,
                   "--extra-flags", str(extra)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                say("round %d, %s: exit %d -- stopping\n%s" % (r, name, p.returncode, p.stdout[-2000:]))
                return p.returncode
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            txt = "round %d  %-26s" % (r, name)
            for where in ("device", "host"):
                med[name][where].append(res[where]["median_ms"])
                txt += "  %s %8.3f ms (min %.3f max %.3f)" % (where, res[where]["median_ms"], res[where]["min_ms"], res[where]["max_ms"])
            say(txt + "  store: %(planes)d planes, %(capacity)d slots" % res["store"])
    say("")
    for where in ("device", "host"):
        m = {k: float(np.median(v[where])) for k, v in med.items()}
        say("%-6s entry point: flag off %.3f ms, flag on %.3f ms per call: (b) / (a) = %.3f" % (where, m[OFF], m[ON], m[ON] / m[OFF]))
        if a.parent_lib:
            pc = 0.5 * (m[P1] + m[P2])
            tol = max([abs(x - y) for x, y in zip(med[P1][where], med[P2][where])] + [abs(m[P1] - m[P2])]) / pc
            d = (m[OFF] - pc) / pc
            say("%-6s entry point: parent %.3f and %.3f ms (its two runs differ by up to %.1f %% within a round), (a) %.3f ms: %+.1f %% "
                "from their mean -> %s" % (where, m[P1], m[P2], 100 * tol, m[OFF], 100 * d,
                                           "within the spread" if abs(d) <= tol else "OUTSIDE the spread"))
    return 0


def idents(addresses, seed=1):
    """One DF 17 identification (valid parity) per address: packed [n, 14] (tools/planes_cost.py)"""
    from gr_adsb_amd import modulator as M
    unit = []
    for i in range(88):
        e = np.zeros(88, np.uint8)
        e[i] = 1
        unit.append(M.crc24(e))
    unit = np.array(unit, np.uint32)
    rng = np.random.default_rng(seed)
    aa = np.asarray(addresses, dtype=np.int64)
    bits = np.zeros((len(aa), 112), np.uint8)
    bits[:, :5] = [1, 0, 0, 0, 1]
    bits[:, 8:32] = (aa[:, None] >> np.arange(23, -1, -1)) & 1
    bits[:, 32:37] = [0, 0, 1, 0, 0]
    bits[:, 40:88] = rng.integers(0, 2, (len(aa), 48))
    par = np.bitwise_xor.reduce(np.where(bits[:, :88].astype(bool), unit[None, :], 0), axis=1)
    bits[:, 88:] = (par[:, None] >> np.arange(23, -1, -1)) & 1
    return np.packbits(bits, axis=1)


def timed(prepare, fn):
    t = []
    for k in range(a.reps + 2):
        prepare()
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))


def expiries():
    from gr_adsb_amd import _native as N
    from gr_adsb_amd import modulator as M
    say("")
    say("(c) adsb_planes_expire: scans 2^24 first-announcement keys = 128 MiB; one read %s us" % scale(8 << 24))
    say("%8s %-12s %30s" % ("planes", "removes", "us"))
    for n in (10 ** 3, 10 ** 5):
        c = N.Context(2e6, 0.0, flags=N.FLAG_AIRCRAFT_TABLE | N.FLAG_DECODE | N.FLAG_PLANE_AGES)
        addr = np.random.default_rng(7).permutation(1 << 24)[:n]
        b, t = idents(addr), 1000.5 + np.zeros(n)
        fill = lambda: c.decode_pdus(b, t)                                             # noqa: E731
        fill()
        say("%8d %-12s %10.1f (%.1f .. %.1f)" % ((n, "none") + timed(lambda: None, lambda: c.expire_planes(0))))
        say("%8d %-12s %10.1f (%.1f .. %.1f)" % ((n, "all") + timed(fill, lambda: c.expire_planes(2000))))
        assert len(c.planes()) == 0
        c.close()
    say("")
    say("(d) adsb_stream_planes_expire: 1024 streams x 24 planes, a rehash of the store (112 bytes a slot) into one of its size")
    say("%8s %8s %-10s %16s %30s" % ("slots", "planes", "removes", "one read us", "us"))
    FS, PER = 2e6, 24
    rng = np.random.default_rng(8)
    rows = np.unpackbits(idents(0x500000 + 4099 * np.arange(PER), seed=2), axis=1)
    z = ((rng.standard_normal(PER * 400 + 1200, dtype=np.float32) + 1j * rng.standard_normal(PER * 400 + 1200, dtype=np.float32)) *
         np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
    for k, bits in enumerate(rows):
        env = M.burst_waveform(bits, 2)
        z[400 + k * 400:400 + k * 400 + len(env)] += env
    for slots in (1 << 16, 1 << 20):
        c = N.Context(FS, 0.05, flags=N.FLAG_STREAM_DECODE | N.FLAG_PLANE_AGES)
        c.open_streams(1024)
        c.set_streams_decoder("Extended Squitter Only")
        c.stream_decoder_reserve(slots)
        fill = lambda: c.process_stream_batch(N.FMT_FC32, list(range(1024)), [z] * 1024, end=True)    # noqa: E731
        fill()
        planes, cap, _ = c.stream_decoder_stats()
        assert planes == 1024 * PER and cap == slots, (planes, cap)
        none, all_ = [-(1 << 62)] * 1024, [1 << 40] * 1024
        say("%8d %8d %-10s %16s %10.1f (%.1f .. %.1f)" % ((cap, planes, "none", scale(112 * cap)) + timed(lambda: None, lambda: c.expire_stream_planes(none))))
        say("%8d %8d %-10s %16s %10.1f (%.1f .. %.1f)" % ((cap, planes, "all", scale(112 * cap)) + timed(fill, lambda: c.expire_stream_planes(all_))))
        assert c.stream_decoder_stats()[0] == 0
        c.close()


def main():
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("plane ages (ADSB_FLAG_PLANE_AGES) on %s" % torch.cuda.get_device_name(0))
    say("decode step: 1024 streams x 2^16-sample uint8 IQ chunks, 2 Msps, 16 consecutive calls; median wall ms per call, %d rounds "
        "of fresh processes, the sides alternated" % a.rounds)
    rc = decode_step()
    if rc == 0:
        expiries()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
