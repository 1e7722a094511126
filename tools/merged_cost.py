"""Cost of the fleet's merged picture (adsb_stream_planes_merged) beside the per-stream snapshot it folds
(adsb_stream_planes_seen) and beside the host alternative (the snapshot plus a NumPy fold), on the fleet of
tools/expire_cost.py (d): 1024 streams x 24 planes = 24576 planes in a store of 65536 slots, every stream selected.
  (1) every stream hears the same 24 aircraft: 24 rows, each folded from 1024 entries (one lane walks 1024 entries);
  (2) the same number of planes, every aircraft shared by 64 streams: 384 rows of 64 entries.
Host clock around the blocking call, median (min .. max) of --reps calls after two that do not count.  Both device calls are
launch-bound: a key scan, 33 sort launches, and one (snapshot) or three (merged) more.
    python tools/merged_cost.py [--reps 25] [--out profiles/planes_merged_cost.txt]
(GPU box only.)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []
FS, PER, STREAMS, SLOTS = 2e6, 24, 1024, 1 << 16


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    t = []
    for k in range(a.reps + 2):
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))


def idents(addresses, seed=1):
    """One DF 17 identification (valid parity) per address: packed [n, 14] (tools/expire_cost.py)"""
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


def chunk(addresses, seed):
    """One stream's samples: an identification of every aircraft, 200 us apart (tools/expire_cost.py (d))"""
    from gr_adsb_amd import modulator as M
    rng = np.random.default_rng(seed)
    rows = list(np.unpackbits(idents(addresses, seed=seed), axis=1))
    n = len(rows) * 400 + 1200
    z = ((rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) *
         np.float32(np.sqrt(1e-4 / 2))).astype(np.complex64)
    for k, bits in enumerate(rows):
        env = M.burst_waveform(bits, 2)
        z[400 + k * 400:400 + k * 400 + len(env)] += env
    return z


def numpy_fold(rows, seen, first):
    """The host alternative: the rule of include/adsb_hip.h (MERGED PICTURE) over adsb_stream_planes_seen's rows"""
    from gr_adsb_amd import _native as N
    stream = np.repeat(np.arange(len(first) - 1), np.diff(first))
    order = np.lexsort((stream, -seen, rows["icao"]))
    icao = rows["icao"][order]
    addr, start = np.unique(icao, return_index=True)
    out = np.zeros(len(addr), dtype=N.DECODED_DTYPE)
    out["icao"], out["present"] = addr, N.DEC_HAS_PLANE
    out["latitude"] = out["longitude"] = np.nan
    out["num_msgs"] = np.add.reduceat(rows["num_msgs"][order].astype(np.uint64), start).astype(np.uint32)
    info = np.zeros(len(addr), dtype=N.MERGED_DTYPE)
    info["last_seen"], info["n_streams"] = seen[order][start], np.diff(np.append(start, len(order)))
    groups = ((rows["present"] & N.DEC_HAS_CALLSIGN) != 0, ("callsign",), N.DEC_HAS_CALLSIGN, "src_callsign"), \
        ((rows["present"] & N.DEC_HAS_ALTITUDE) != 0, ("altitude",), N.DEC_HAS_ALTITUDE, "src_altitude"), \
        ((rows["present"] & N.DEC_HAS_VELOCITY) != 0, ("velocity_we", "velocity_sn", "vertical_rate"), N.DEC_HAS_VELOCITY, "src_velocity"), \
        (~np.isnan(rows["latitude"]), ("latitude", "longitude"), 0, "src_position")
    for has, fields, flag, src in groups:
        info[src] = -1
        pick = order[has[order]]                      # the entries that have the group, freshest first inside an address
        got, at = np.unique(rows["icao"][pick], return_index=True)
        j = np.searchsorted(addr, got)
        for k in fields:
            out[k][j] = rows[k][pick[at]]
        out["present"][j] |= flag
        info[src][j] = stream[pick[at]]
    return out, info


def fleet(shared_by):
    from gr_adsb_amd import _native as N
    c = N.Context(FS, 0.05, flags=N.FLAG_STREAM_DECODE | N.FLAG_PLANE_AGES)
    c.open_streams(STREAMS)
    c.set_streams_decoder("Extended Squitter Only")
    c.stream_decoder_reserve(SLOTS)
    groups = STREAMS // shared_by
    zs = [chunk(0x500000 + 4099 * (np.arange(PER) + PER * g), seed=2 + g) for g in range(groups)]
    for s in range(STREAMS):
        c.set_stream_start(s, 1000.5 + s % 7)
    c.process_stream_batch(N.FMT_FC32, list(range(STREAMS)), [zs[s // shared_by] for s in range(STREAMS)], end=True)
    planes, cap, _ = c.stream_decoder_stats()
    assert planes == STREAMS * PER and cap == SLOTS, (planes, cap)
    rows, info = c.merged_planes()
    assert len(rows) == PER * groups and (info["n_streams"] == shared_by).all()
    er, ei = numpy_fold(*c.stream_planes(seen=True))
    assert er.tobytes() == rows.tobytes() and ei.tobytes() == info.tobytes(), "the NumPy fold and the device disagree"
    n = len(rows)
    snap = timed(lambda: c.stream_planes(cap=planes, seen=True))
    merged = timed(lambda: c.merged_planes(cap=n))
    host = timed(lambda: numpy_fold(*c.stream_planes(cap=planes, seen=True)))
    say("%6d aircraft x %4d streams  %-44s %9.1f us (%.1f .. %.1f)" % ((n, shared_by, "adsb_stream_planes_seen (24576 rows)") + snap))
    say("%6d aircraft x %4d streams  %-44s %9.1f us (%.1f .. %.1f)" % ((n, shared_by, "adsb_stream_planes_merged (%d rows)" % n) + merged))
    say("%6d aircraft x %4d streams  %-44s %9.1f us (%.1f .. %.1f)" % ((n, shared_by, "adsb_stream_planes_seen + NumPy fold") + host))
    say("       merged / snapshot = %.2f, host alternative / merged = %.1f" % (merged[0] / snap[0], host[0] / merged[0]))
    c.close()


def main():
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("the fleet's merged picture (adsb_stream_planes_merged) on %s" % torch.cuda.get_device_name(0))
    say("1024 streams, 24576 planes, 65536 slots, every stream selected, cutoff INT64_MIN; host clock around the blocking call, "
        "median (min .. max) of %d calls" % a.reps)
    fleet(STREAMS)
    fleet(64)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
