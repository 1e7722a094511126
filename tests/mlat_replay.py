"""MULTILATERATION of include/adsb_hip.h restated in plain Python / NumPy, from the header's text alone: the group rule over a
carry given as a list of (ts, payload, stream) in carry order, and the solver in a float type of the caller's choice --
float64, the rule's own, and np.longdouble, which tells how far the float64 result is its own rounding (the tolerance of
tests/test_mlat.py and tests/test_gpu_mlat.py).  Nothing here knows the device code."""
import numpy as np

C = 299702547.0
OK, NO_CONVERGE, SINGULAR = 0, 1, 2
MAX_CAND, MAX_ITER = 64, 32
POLY = 0x1FFF409


def payload_of(bits14, long_):
    """The payload the rule compares: (length marker, the masked bytes); None for an entry that takes no part is the caller's."""
    b = bytes(bytearray(np.asarray(bits14, np.uint8).tolist()))
    return (2, b[:14]) if long_ else (1, b[:7])


def groups(carry, window):
    """carry: [(ts, payload or None, stream)] in carry order -> [(head index, [member indices, the head first])], in carry
    order of the heads.  O(n * entries within the window), by the rule's two tests as the header spells them."""
    n = len(carry)
    out = []
    for i in range(n):
        ts_i, pay_i, _ = carry[i]
        if pay_i is None:
            continue
        head = True
        q = i - 1
        while q >= 0:
            ts_q, pay_q, _ = carry[q]
            if not (np.float64(ts_i) - np.float64(ts_q) <= window):
                break                                                  # the carry is sorted: nothing further in front is nearer
            if pay_q is not None and pay_q == pay_i:
                head = False
                break
            q -= 1
        if not head:
            continue
        members = [i]
        for m in range(i + 1, n):
            ts_m, pay_m, _ = carry[m]
            if not (np.float64(ts_m) - np.float64(ts_i) <= window):
                break
            if pay_m is not None and pay_m == pay_i:
                members.append(m)
        out.append((i, members))
    return out


def used_of(carry, members, positioned):
    """-> the used hearings (indices into the carry): of the first 64 members the first of each stream, if it has a position"""
    seen, used = set(), []
    for m in members[:MAX_CAND]:
        s = carry[m][2]
        if s in seen:
            continue
        seen.add(s)
        if positioned(s):
            used.append(m)
    return used


def remainder(bits, nbits):
    v = 0
    for i in range(nbits):
        v = (v << 1) | ((bits[i >> 3] >> (7 - (i & 7))) & 1)
        if v & 0x1000000:
            v ^= POLY
    return v


def icao_of(payload):
    marker, b = payload
    df = b[0] >> 3
    if df in (11, 17, 18):
        return (b[1] << 16) | (b[2] << 8) | b[3]
    if df in (0, 4, 5, 16, 20, 21):
        return remainder(b, 112 if marker == 2 else 56)
    return -1


def solve(R, ts, ts_head, ft=np.float64):
    """R: (n, 3) receivers of the used hearings in carry order; ts: their arrival times -> dict(p, b, t_tx, rms_m, status, iters)"""
    R = np.asarray(R, np.float64).astype(ft)
    n = len(R)
    c_ = ft(C)
    d = c_ * (np.asarray(ts, np.float64) - np.float64(ts_head)).astype(ft)      # the difference first, in double
    cen = R.sum(axis=0) / ft(n)
    p = cen + ft(10000.0) * (cen / np.sqrt((cen * cen).sum()))
    b = np.sqrt(((p - R[0]) ** 2).sum())
    status, iters = NO_CONVERGE, 0
    with np.errstate(all="ignore"):
        for _ in range(MAX_ITER):
            diff = p[None, :] - R
            rho = np.sqrt((diff * diff).sum(axis=1))
            u = diff / rho[:, None]
            r = rho - d - b
            J = np.concatenate([u, -np.ones((n, 1), ft)], axis=1)
            A = J.T @ J
            A[3, 3] = ft(n)
            g = J.T @ r
            L = np.zeros((4, 4), ft)
            bad = False
            for j in range(4):
                piv = A[j, j] - (L[j, :j] * L[j, :j]).sum()
                if not (piv > 0 and np.isfinite(piv)):
                    bad = True
                    break
                L[j, j] = np.sqrt(piv)
                for i in range(j + 1, 4):
                    L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
            if bad:
                status = SINGULAR
                break
            y = np.zeros(4, ft)
            for i in range(4):
                y[i] = (-g[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
            delta = np.zeros(4, ft)
            for i in range(3, -1, -1):
                delta[i] = (y[i] - (L[i + 1:, i] * delta[i + 1:]).sum()) / L[i, i]
            p = p + delta[:3]
            b = b + delta[3]
            iters += 1
            if np.sqrt((delta[:3] * delta[:3]).sum()) < ft(1e-3):
                status = OK
                break
        diff = p[None, :] - R
        r = np.sqrt((diff * diff).sum(axis=1)) - d - b
        rms = np.sqrt((r * r).sum() / ft(n))
    return dict(p=p, b=b, t_tx=ft(ts_head) - b / c_, rms_m=rms, status=status, iters=iters)


def mlat(carry, window, rx, t_lo=-np.inf, t_hi=np.inf, min_rx=4, ft=np.float64):
    """carry as for groups(); rx: {stream: (x, y, z)} -> (fixes: list of dicts, member_stream, member_ts), the rows
    adsb_stream_mlat returns: heads with t_lo <= ts < t_hi and n_rx >= min_rx, in carry order."""
    fixes, mstream, mts = [], [], []
    for h, members in groups(carry, window):
        ts_h = carry[h][0]
        if not (t_lo <= ts_h < t_hi):
            continue
        used = used_of(carry, members, lambda s: s in rx)
        if len(used) < min_rx:
            continue
        R = np.array([rx[carry[m][2]] for m in used], np.float64)
        sol = solve(R, [carry[m][0] for m in used], ts_h, ft)
        marker, b = carry[h][1]
        sol.update(ts=ts_h, bits=np.frombuffer(b + bytes(14 - len(b)), np.uint8), flags=64 if marker == 2 else 0, icao=icao_of(carry[h][1]),
                   n_rx=len(used), n_heard=len(members), first=len(mstream), head=h, used=used)
        fixes.append(sol)
        mstream += [carry[m][2] for m in used]
        mts += [carry[m][0] for m in used]
    return fixes, np.array(mstream, np.int32), np.array(mts, np.float64)


# ---- WGS-84, for the tests' worlds and the helpers' own check ----------------------------------------------------------------
WGS_A, WGS_F = 6378137.0, 1.0 / 298.257223563


def geodetic_to_ecef(lat_deg, lon_deg, alt_m, ft=np.float64):
    a, f = ft(WGS_A), ft(1) / ft(298.257223563)
    e2 = f * (ft(2) - f)
    lat, lon = np.deg2rad(ft(lat_deg)), np.deg2rad(ft(lon_deg))
    sl, cl = np.sin(lat), np.cos(lat)
    n = a / np.sqrt(ft(1) - e2 * sl * sl)
    alt = ft(alt_m)
    return np.array([(n + alt) * cl * np.cos(lon), (n + alt) * cl * np.sin(lon), (n * (ft(1) - e2) + alt) * sl], ft)
