"""Cost of a plane snapshot (adsb_planes, adsb_stream_planes), host clock around the blocking call (it ends in a stream
synchronise and includes the copy of the rows to the host); median, minimum and maximum of --reps calls after three warm-up calls.
  dense: an ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE context holding 10^3 and 10^5 planes (DF 17 identifications of as many
    addresses through adsb_decode_pdus): the count query (tally and scan only) and the whole snapshot.
  fleet: 1024 receiver streams on an ADSB_FLAG_STREAM_DECODE context, every stream hearing the same 24 aircraft: the store at its
    initial size, and after a second call with 24 more has made it grow once; all streams, and one stream.
Beside each figure, for scale: the time ONE read of the scanned array (the 2^24 first-announcement keys, the store's keys)
takes at the read-only ceiling DESIGN.md section 6 records (0.843-0.874 of 8 TB/s).
    python tools/planes_cost.py [--reps 25] [--out FILE]            (needs the GPU)"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from gr_adsb_amd import _native as N  # noqa: E402
from gr_adsb_amd import modulator as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 20
lines = []
CEILING = (0.843 * 8e12, 0.874 * 8e12)        # bytes / s


def say(s):
    print(s, flush=True)
    lines.append(s)


_R = []
for i in range(88):
    e = np.zeros(88, np.uint8)
    e[i] = 1
    _R.append(M.crc24(e))
_R = np.array(_R, np.uint32)


def idents(addresses, seed=1):
    """One DF 17 identification (valid parity) per address: packed [n, 14]"""
    rng = np.random.default_rng(seed)
    aa = np.asarray(addresses, dtype=np.int64)
    bits = np.zeros((len(aa), 112), np.uint8)
    bits[:, :5] = [1, 0, 0, 0, 1]
    bits[:, 8:32] = (aa[:, None] >> np.arange(23, -1, -1)) & 1
    bits[:, 32:37] = [0, 0, 1, 0, 0]
    bits[:, 40:88] = rng.integers(0, 2, (len(aa), 48))
    par = np.bitwise_xor.reduce(np.where(bits[:, :88].astype(bool), _R[None, :], 0), axis=1)
    bits[:, 88:] = (par[:, None] >> np.arange(23, -1, -1)) & 1
    return np.packbits(bits, axis=1)


def timed(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))


def scale(nbytes):
    return "%.2f-%.2f" % (nbytes / CEILING[1] * 1e6, nbytes / CEILING[0] * 1e6)


import torch  # noqa: E402
assert torch.cuda.is_available(), "this measurement needs the GPU"
say("plane snapshots: us per call, median (min .. max) of %d calls; 'one read' = the scanned array once at the read-only ceiling" % a.reps)
say("")
say("dense (adsb_planes): scans 2^24 first-announcement keys = 128 MiB; one read %s us" % scale(8 << 24))
say("%8s %-12s %30s" % ("planes", "call", "us"))
for n in (10 ** 3, 10 ** 5):
    c = N.Context(2e6, 0.0, flags=N.FLAG_AIRCRAFT_TABLE | N.FLAG_DECODE)
    addr = np.random.default_rng(7).permutation(1 << 24)[:n]
    c.decode_pdus(idents(addr), 1760000000.0 + 1e-3 * np.arange(n))
    assert len(c.planes()) == n
    cnt = ctypes.c_int32(0)
    say("%8d %-12s %10.1f (%.1f .. %.1f)" % ((n, "count query") + timed(lambda: c.lib.adsb_planes(c._h, None, 0, ctypes.byref(cnt)))))
    assert cnt.value == n
    say("%8d %-12s %10.1f (%.1f .. %.1f)" % ((n, "snapshot") + timed(lambda: c.planes(cap=n))))
    c.close()
say("")
say("fleet (adsb_stream_planes): 1024 streams, scans the store's 8-byte keys")
say("%8s %8s %-12s %12s %30s" % ("slots", "planes", "selection", "one read us", "us"))
FS, PER = 2e6, 24
c = N.Context(FS, 0.05, flags=N.FLAG_STREAM_DECODE)
c.open_streams(1024)
c.set_streams_decoder("Extended Squitter Only")
rng = np.random.default_rng(8)
for call in range(2):
    rows = np.unpackbits(idents(0x500000 + 4099 * (PER * call + np.arange(PER)), seed=2 + call), axis=1)
    step = 400
    z = ((rng.standard_normal(PER * step + 1200, dtype=np.float32) + 1j * rng.standard_normal(PER * step + 1200, dtype=np.float32)) *
         np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
    for k, b in enumerate(rows):
        env = M.burst_waveform(b, 2)
        z[400 + k * step:400 + k * step + len(env)] += env
    c.process_stream_batch(N.FMT_FC32, list(range(1024)), [z] * 1024, end=True)
    planes, cap, grows = c.stream_decoder_stats()
    assert planes == 1024 * PER * (call + 1) and grows == call, (planes, cap, grows)
    for name, sel in (("all streams", None), ("one stream", [512])):
        r, f = c.stream_planes(sel)
        assert len(r) == (planes if sel is None else PER * (call + 1))
        say("%8d %8d %-12s %12s %10.1f (%.1f .. %.1f)" % ((cap, planes, name, scale(8 * cap)) + timed(lambda: c.stream_planes(sel, cap=len(r)))))
c.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
