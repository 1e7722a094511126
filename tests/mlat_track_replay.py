"""The MLAT TRACKS rule of include/adsb_hip.h, restated in plain Python: steps 1 to 5, fix by fix, with float64 scalars and the
header's order of operations, on (fixes, aux) arrays and a dict of tracks by address.  The rule is sequential per address and
every expression has one order, so the kernels must equal this byte for byte: no test that uses it has a tolerance.

A track is a dict with adsb_mlat_track's fields.  update() takes the fixes in row order, which per address is the order the
device walks them in (the key sort is stable and keyed by (icao, row))."""
import math

import numpy as np

OK = 0
GAP, RESTARTED = 1, 2
DEFAULTS = dict(alpha=0.3, beta=0.05, gate_m=2000.0, max_speed_mps=350.0, max_gap_s=30.0, max_rms_m=500.0, min_up_m=0.0, restart_after=3)
STATS = ("fixes", "eligible", "unusable", "stale", "rejected", "taken", "started", "tracks")
F = np.float64


def usable(f, up_m, R):
    return (int(f["status"]) == OK and all(math.isfinite(float(f[k])) for k in ("x", "y", "z", "rms_m")) and
            F(f["rms_m"]) <= F(R["max_rms_m"]) and F(up_m) >= F(R["min_up_m"]))


def start(T, f):
    T.update(x=F(f["x"]), y=F(f["y"]), z=F(f["z"]), vx=F(0), vy=F(0), vz=F(0), first_ts=F(f["ts"]), last_ts=F(f["ts"]), n_fixes=1, misses=0,
             rms_m=F(f["rms_m"]), n_rx=int(f["n_rx"]))


def update(tracks, fixes, aux, rule):
    """tracks: {icao: track}, changed in place; aux: the aux rows or None (up_m 0) -> the call's stats as a dict"""
    R = dict(DEFAULTS)
    R.update(rule)
    alpha, beta, gate, vmax, gap = (F(R[k]) for k in ("alpha", "beta", "gate_m", "max_speed_mps", "max_gap_s"))
    s = dict.fromkeys(STATS, 0)
    s["fixes"] = len(fixes)
    for row in range(len(fixes)):
        f = fixes[row]
        icao = int(f["icao"])
        if icao < 0:
            continue
        s["eligible"] += 1
        if not usable(f, aux[row]["up_m"] if aux is not None else 0.0, R):                     # 1. USABLE
            s["unusable"] += 1
            continue
        T = tracks.get(icao)
        ts = F(f["ts"])
        if T is not None and ts <= T["last_ts"]:                                                # 2. STALE
            s["stale"] += 1
            continue
        if T is None or ts - T["last_ts"] > gap:                                                # 3. START
            if T is None:
                T = tracks[icao] = dict(icao=icao, flags=0, n_rejected=0)
            else:
                T["flags"] |= GAP
            start(T, f)
            s["started"] += 1
            continue
        dt = ts - T["last_ts"]                                                                  # 4. GATE
        ppx, ppy, ppz = T["x"] + T["vx"] * dt, T["y"] + T["vy"] * dt, T["z"] + T["vz"] * dt
        dx, dy, dz = F(f["x"]) - ppx, F(f["y"]) - ppy, F(f["z"]) - ppz
        dist = F(math.sqrt(dx * dx + dy * dy + dz * dz))
        if dist > gate + vmax * dt:
            T["n_rejected"] += 1
            T["misses"] += 1
            s["rejected"] += 1
            if T["misses"] >= int(R["restart_after"]):
                T["flags"] |= RESTARTED
                start(T, f)
                s["started"] += 1
            continue
        gv = beta / dt                                                                          # 5. STEP
        T["x"], T["y"], T["z"] = ppx + alpha * dx, ppy + alpha * dy, ppz + alpha * dz
        T["vx"], T["vy"], T["vz"] = T["vx"] + gv * dx, T["vy"] + gv * dy, T["vz"] + gv * dz
        T["last_ts"] = ts
        T["n_fixes"] += 1
        T["misses"] = 0
        T["rms_m"], T["n_rx"] = F(f["rms_m"]), int(f["n_rx"])
        s["taken"] += 1
    s["tracks"] = len(tracks)
    return s


def rows(tracks, dtype, min_fixes=None, cutoff=-np.inf):
    """the store as the device holds and reads it: ascending icao; min_fixes None: every track (the store itself)"""
    keep = [T for _, T in sorted(tracks.items()) if (min_fixes is None or T["n_fixes"] >= min_fixes) and T["last_ts"] >= cutoff]
    out = np.zeros(len(keep), dtype=dtype)
    for k, T in enumerate(keep):
        for name in dtype.names:
            out[k][name] = T[name]
    return out


def from_rows(rows_):
    """the inverse of rows(): a dict of tracks with float64 / int fields"""
    out = {}
    for r in rows_:
        T = {}
        for name in rows_.dtype.names:
            T[name] = F(r[name]) if rows_.dtype[name].kind == "f" else int(r[name])
        out[T["icao"]] = T
    return out


def expire(tracks, cutoff):
    gone = [a for a, T in tracks.items() if T["last_ts"] < cutoff]
    for a in gone:
        del tracks[a]
    return len(gone)
