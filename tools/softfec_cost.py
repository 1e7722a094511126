"""Cost of the soft-decision CRC repair (ADSB_FLAG_FEC_SOFT), by the method of tools/mlat_track_cost.py: every side is a fresh
child process under a time limit of its own, the sides alternated, three rounds, medians; the first non-zero exit ends the run.
One blocking adsb_process_format_device pass over a bench-like 2^26-sample complex64 stream at 2 Msps that lies in device memory:
  (v) parity-consistent DF 17 replies at 6..14 dB over noise (modulator.synth_iq, made on the host and uploaded): the share of
      records that qualify is that of a weak-signal receiver in this synthetic model;
  (w) random payloads (the bench's own stream): every DF 17 record fails parity and qualifies -- the worst case.
Sides: the flag off on the PARENT commit's build (--parent-lib; run twice per round: the spread this build is held against) and
on this build; ADSB_FLAG_FEC_CONSERVATIVE alone; Conservative plus soft at 8 / 3 and at 16 / 5, reported against the
Conservative-only pass, with the share of records that qualified and the number repaired.  No figure is fixed in advance.
    python tools/softfec_cost.py --parent-lib /path/to/parent/libadsb_hip.so [--rounds 3] [--out profiles/softfec_cost.txt]
(GPU box only.)"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--log2n", type=int, default=26)
ap.add_argument("--passes", type=int, default=30)
ap.add_argument("--child", default=None)                 # "<flags>:<n_weak>:<max_flips>"
ap.add_argument("--stream", choices=["v", "w"], default="v")
ap.add_argument("--lib", default=None)
ap.add_argument("--child-timeout", type=int, default=180)
a = ap.parse_args()

FS, THR, F, S = 2e6, 0.004, 128, 16384
N = 1 << a.log2n


def child():
    """one process, one library, one flag set -> one JSON line"""
    import time
    import numpy as np
    import torch
    from gr_adsb_amd import modulator as M
    flags, n_weak, max_flips = (int(v) for v in a.child.split(":"))
    c = ctypes
    lib = c.CDLL(a.lib)
    vp, i32, i64 = c.c_void_p, c.c_int32, c.c_int64
    lib.adsb_create.argtypes = [c.c_double, c.c_float, c.c_int, c.c_uint32, c.POINTER(vp)]
    lib.adsb_destroy.argtypes = [vp]
    lib.adsb_destroy.restype = None
    lib.adsb_process_format_device.argtypes = [vp, c.c_int, vp, i64, i64, vp, i32, c.POINTER(i32)]
    h = vp()
    assert lib.adsb_create(FS, THR, 0, flags, c.byref(h)) == 0
    if flags & S:
        class Rule(c.Structure):
            _fields_ = [("n_weak", i32), ("max_flips", i32), ("min_key", c.c_float), ("flags", c.c_uint32)]
        lib.adsb_set_soft_fec.argtypes = [vp, c.POINTER(Rule)]
        lib.adsb_last_soft.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
        assert lib.adsb_set_soft_fec(h, c.byref(Rule(n_weak, max_flips, 0.0, 0))) == 0
    dev = torch.device("cuda:0")
    blk = 1 << 24
    if a.stream == "v":
        z = M.synth_iq(N, FS, 1500, 0, noise_power=1e-3, snr_db_range=(6, 14))
        iq = torch.from_numpy(z.view(np.float32).reshape(-1, 2)).to(dev).contiguous()
    else:
        iq = torch.cat([M.synth_iq_torch(blk, FS, 1500.0, 200 + b, dev, snr_db_range=(6, 14)) for b in range(N // blk)]).contiguous()
    torch.cuda.synchronize()
    n_out = i32(0)
    ms = []
    for k in range(a.passes + 3):
        t0 = time.perf_counter()
        rc = lib.adsb_process_format_device(h, 0, vp(iq.data_ptr()), N, 0, None, 0, c.byref(n_out))
        t1 = time.perf_counter()
        assert rc == 0, rc
        if k >= 3:
            ms.append((t1 - t0) * 1e3)
    res = {"ms": float(np.median(ms)), "lo": float(np.min(ms)), "records": int(n_out.value)}
    if flags & S:
        p, n = vp(), i32(0)
        assert lib.adsb_last_soft(h, c.byref(p), c.byref(n)) == 0
        rows = np.frombuffer((c.c_char * (n.value * 8)).from_address(p.value), dtype=np.uint8).reshape(-1, 8)
        res["qualified"] = int((rows[:, 1] > 0).sum())
        res["repaired"] = int((rows[:, 0] > 0).sum())
    lib.adsb_destroy(h)
    print(json.dumps(res))


def run_child(lib, stream, spec):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", spec, "--lib", lib, "--stream", stream, "--log2n", str(a.log2n),
           "--passes", str(a.passes)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit("child %s exited with %d: the run ends here" % (spec, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    import numpy as np
    this = os.path.join(ROOT, "gr_adsb_amd", "libadsb_hip.so")
    sides = [("this: flag off", this, "0:8:3"), ("this: Conservative", this, "%d:8:3" % F),
             ("this: Conservative + soft 8/3", this, "%d:8:3" % (F | S)), ("this: Conservative + soft 16/5", this, "%d:16:5" % (F | S))]
    if a.parent_lib:
        sides = [("parent: flag off (a)", a.parent_lib, "0:8:3")] + sides + [("parent: flag off (b)", a.parent_lib, "0:8:3")]
    lines = ["soft-decision CRC repair: one blocking adsb_process_format_device pass, complex64, 2^%d samples at 2 Msps, median of %d passes"
             % (a.log2n, a.passes), "per child, median over %d rounds of fresh children, sides alternated; ms per pass" % a.rounds]
    for stream, what in (("v", "(v) parity-consistent DF 17 replies at 6..14 dB"), ("w", "(w) random payloads: every DF 17 record qualifies")):
        got = {name: [] for name, _, _ in sides}
        for _ in range(a.rounds):
            for name, lib, spec in sides:
                got[name].append(run_child(lib, stream, spec))
        lines.append("")
        lines.append(what)
        med = {name: float(np.median([g["ms"] for g in v])) for name, v in got.items()}
        for name, _, _ in sides:
            v = got[name]
            text = "  %-34s %8.3f ms   rounds: %s   records %d" % (name, med[name], " ".join("%.3f" % g["ms"] for g in v), v[-1]["records"])
            if "qualified" in v[-1]:
                text += "   qualified %d (%.1f %%)   repaired %d   vs Conservative alone %+.3f ms (%+.2f %%)" % (
                    v[-1]["qualified"], 100.0 * v[-1]["qualified"] / max(1, v[-1]["records"]), v[-1]["repaired"],
                    med[name] - med["this: Conservative"], 100.0 * (med[name] / med["this: Conservative"] - 1.0))
            lines.append(text)
        if a.parent_lib:
            pa, pb = med["parent: flag off (a)"], med["parent: flag off (b)"]
            lines.append("  flag off, this build against the parent's two runs: %+.3f / %+.3f ms; the parent against itself: %+.3f ms"
                         % (med["this: flag off"] - pa, med["this: flag off"] - pb, pb - pa))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    child() if a.child else main()
