"""THE DAMPED RULE, THE RESTART and THE ALTITUDE ROW of include/adsb_hip.h (MULTILATERATION) restated in plain Python / NumPy, from
the header's text alone, in a float type of the caller's choice -- float64, the rule's own, and np.longdouble, which tells how
far the float64 result is its own rounding (the tolerance of tests/test_mlat_rule.py).  The group rule, the used hearings and
the row's other fields are tests/mlat_replay.py's.  Nothing here knows the device code."""
import numpy as np

import mlat_replay as MR

C = MR.C
OK, NO_CONVERGE, SINGULAR = MR.OK, MR.NO_CONVERGE, MR.SINGULAR
SOLVER_GN, SOLVER_LM = 0, 1
RESTART, ALTITUDE = 1, 2
AUX_AIDED, AUX_RESTARTED, AUX_SECOND_KEPT = 1, 2, 4
MAX_TRIALS = 64


def field(b, lo, n):
    """bits lo .. lo + n - 1 of the reply whose bytes are b, the first bit of a byte its most significant"""
    v = 0
    for i in range(lo, lo + n):
        v = (v << 1) | ((b[i >> 3] >> (7 - (i & 7))) & 1)
    return v


def alt_ft_of(payload):
    """The altitude the payload announces, by the header's text -> feet, or -1"""
    _, b = payload
    df = b[0] >> 3
    if df in (0, 4, 16, 20):
        v = field(b, 19, 13)
        if v == 0 or v & 0x40 or not v & 0x10:
            return -1
        return (((v >> 7) << 5) | (((v >> 5) & 1) << 4) | (v & 0xF)) * 25 - 1000
    if df == 17 and 9 <= field(b, 32, 5) <= 18:
        v = field(b, 40, 12)
        if not v & 0x10:
            return -1
        return (((v >> 5) << 4) | (v & 0xF)) * 25 - 1000
    return -1


def height(p, ft=np.float64):
    """ONE Bowring step -> (h, n)"""
    a = ft(MR.WGS_A)
    f = ft(1) / ft(298.257223563)
    e2 = f * (ft(2) - f)
    bp = a * (ft(1) - f)
    ep2 = e2 / (ft(1) - e2)
    x, y, z = p
    q = np.sqrt(x * x + y * y)
    t = (z * a) / (q * bp)
    cb = ft(1) / np.sqrt(ft(1) + t * t)
    sb = t * cb
    T = (z + ep2 * bp * (sb * sb * sb)) / (q - e2 * a * (cb * cb * cb))
    cp = ft(1) / np.sqrt(ft(1) + T * T)
    sp = T * cp
    h = q * cp + z * sp - a * np.sqrt(ft(1) - e2 * (sp * sp))
    return h, np.array([cp * (x / q), cp * (y / q), sp], ft)


def run(R, d, start, alt, ft):
    """A damped run.  alt: None or (w, h_want) -> dict(p, b, status, iters, tries, lam)"""
    n = len(R)
    p = start.copy()
    b = np.sqrt(((p - R[0]) ** 2).sum())
    lam = ft(1e-3)

    def rows(p, b):
        diff = p[None, :] - R
        rho = np.sqrt((diff * diff).sum(axis=1))
        r = rho - d - b
        if alt is None:
            return diff, rho, r, None, ft(0)
        h, nrm = height(p, ft)
        return diff, rho, r, alt[0] * nrm, alt[0] * (h - alt[1])

    def total(r, ra):
        return (r * r).sum() + ra * ra

    _, _, r, _, ra = rows(p, b)
    S = total(r, ra)
    status, iters, tries = NO_CONVERGE, 0, 0
    for _ in range(MAX_TRIALS):
        diff, rho, r, ja, ra = rows(p, b)
        u = diff / rho[:, None]
        J = np.concatenate([u, -np.ones((n, 1), ft)], axis=1)
        A = J.T @ J
        A[3, 3] = ft(n)
        g = J.T @ r
        if ja is not None:
            A[:3, :3] += ja[:, None] * ja[None, :]
            g[:3] += ja * ra
        for j in range(4):
            A[j, j] = A[j, j] * (ft(1) + lam)
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
        tries += 1
        p1, b1 = p + delta[:3], b + delta[3]
        if lam <= ft(1e-3) and np.sqrt((delta[:3] * delta[:3]).sum()) < ft(1e-3):
            p, b = p1, b1                             # the untested last step
            iters += 1
            status = OK
            break
        _, _, r1, _, ra1 = rows(p1, b1)
        S1 = total(r1, ra1)
        if np.isfinite(S1) and S1 <= S:
            p, b, S = p1, b1, S1
            iters += 1
            lam = max(lam / ft(10), ft(1e-12))
            if np.sqrt((delta[:3] * delta[:3]).sum()) < ft(1e-3):
                status = OK
                break
        else:
            lam = lam * ft(10)
            if lam > ft(1e12):
                break
    return dict(p=p, b=b, status=status, iters=iters, tries=tries, lam=lam)


def solve(R, ts, ts_head, flags=RESTART, alt_ft=-1, alt_weight=1.0, ft=np.float64):
    """R: (n, 3) receivers of the used hearings in carry order; ts: their arrival times; alt_ft: the head's altitude or -1 (the
    caller passes -1 without ALTITUDE) -> dict(p, b, t_tx, rms_m, status, iters, tries, lam, up_m, aux_flags, alt_ft,
    first_status: how the first run ended)"""
    R = np.asarray(R, np.float64).astype(ft)
    n = len(R)
    c_ = ft(C)
    d = c_ * (np.asarray(ts, np.float64) - np.float64(ts_head)).astype(ft)
    cen = R.sum(axis=0) / ft(n)
    u = cen / np.sqrt((cen * cen).sum())
    up = lambda p: ((p - cen) * u).sum()      # noqa: E731
    aided = alt_ft != -1
    alt = (ft(alt_weight), ft(0.3048) * ft(alt_ft)) if aided else None
    aux = AUX_AIDED if aided else 0
    with np.errstate(all="ignore"):
        keep = run(R, d, cen + ft(10000.0) * u, alt, ft)
        tries, first_status = keep["tries"], keep["status"]
        good = keep["status"] == OK and up(keep["p"]) >= 0
        if flags & RESTART and not aided and not good:
            aux |= AUX_RESTARTED
            start = keep["p"] - (ft(2) * up(keep["p"])) * u if keep["status"] == OK else cen + ft(30000.0) * u
            second = run(R, d, start, alt, ft)
            tries += second["tries"]
            if second["status"] == OK and up(second["p"]) >= 0:
                keep = second
                aux |= AUX_SECOND_KEPT
        p, b = keep["p"], keep["b"]
        diff = p[None, :] - R
        r = np.sqrt((diff * diff).sum(axis=1)) - d - b
        rms = np.sqrt((r * r).sum() / ft(n))
        return dict(p=p, b=b, t_tx=ft(ts_head) - b / c_, rms_m=rms, status=keep["status"], iters=keep["iters"], tries=tries, lam=keep["lam"],
                    up_m=up(p), aux_flags=aux, alt_ft=alt_ft, first_status=first_status)


def mlat(carry, window, rx, t_lo=-np.inf, t_hi=np.inf, solver=SOLVER_LM, flags=RESTART, min_rx=4, alt_weight=1.0, ft=np.float64):
    """adsb_stream_mlat_rule's rows: MR.mlat's selection, but a group of three used hearings only with an altitude, and the
    rule's solve -> (fixes: list of dicts, member_stream, member_ts)"""
    if solver == SOLVER_GN:
        return MR.mlat(carry, window, rx, t_lo, t_hi, min_rx, ft)
    fixes, mstream, mts = [], [], []
    for h, members in MR.groups(carry, window):
        ts_h = carry[h][0]
        if not (t_lo <= ts_h < t_hi):
            continue
        used = MR.used_of(carry, members, lambda s: s in rx)
        alt_ft = alt_ft_of(carry[h][1]) if flags & ALTITUDE else -1
        if len(used) < min_rx or (len(used) == 3 and alt_ft == -1):
            continue
        R = np.array([rx[carry[m][2]] for m in used], np.float64)
        sol = solve(R, [carry[m][0] for m in used], ts_h, flags, alt_ft, alt_weight, ft)
        marker, b = carry[h][1]
        sol.update(ts=ts_h, bits=np.frombuffer(b + bytes(14 - len(b)), np.uint8), flags=64 if marker == 2 else 0, icao=MR.icao_of(carry[h][1]),
                   n_rx=len(used), n_heard=len(members), first=len(mstream), head=h, used=used)
        fixes.append(sol)
        mstream += [carry[m][2] for m in used]
        mts += [carry[m][0] for m in used]
    return fixes, np.array(mstream, np.int32), np.array(mts, np.float64)
