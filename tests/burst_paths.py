"""Streams that make k_detect and k_longrun build burst records through their rarely taken routes (adsb_device.h, enum
Route), shared by the emulator (test_sim_burst_paths.py), the GPU (test_gpu_burst_paths.py) and the reference fixtures
(tools/make_golden_paths.py):

  * long-pulse bursts -- a carrier above the threshold with a preamble whose chip 0 sits on the run's centre
    p = (rise + fall) // 2 (framer.py:113) and data bits after it: the record is built by k_longrun (burst_issue /
    burst_finish) from global memory once the run leaves the LDS window of the tile it rose in, by k_detect otherwise;
  * preamble trains 8 - 12 symbols apart (plus overlapping DF17 replies): more bursts waiting for their bit samples than a
    wavefront's pending list holds (kMaxPend = 8), so k_detect slices the ninth and later ones from global memory, and
    lists that are still full at a wavefront's chunk end (pend_flush).

Every stream is built from integer I / Q components (LSB units, edge_cases.encode turns them into each wire format) and
asserts its own premise on the oracle's |IQ|^2.  The float-only stream signed_zero_runs() is |IQ|^2 at thr 0.0.

Not generated: the virtual rise of k_detect (a unit 0 whose scan starts in the zero history, scan_lo < 0, at thr <= 0 with a
previous sample below the threshold).  No entry point reaches it: the plans with scan_lo < 0 (canonical call, shards) all
start from prev_in0 = 0.0, which is >= every thr <= 0, and the framer's own plan starts its scan at 0.
test_sim_burst_paths.py runs it through the kernel's argument block instead.  That is also the only way to a k_longrun
centre within 100 samples of in0[0] (burst_finish's clamp of the noise window at in0_base): a real rise is at in0[0] at the
earliest, and a run that leaves the LDS window of its rise tile is more than kFwd = 256 samples long, so its centre lies
more than 128 samples after the rise.  Centres near the start of a call or stream are built by k_detect, whose clipped
windows the edge cases and the fixtures' chunked schedules cover."""
import numpy as np

from gr_adsb_amd import modulator as M
from oracle import adsb_oracle as O

# simlib.kernel_geometry() (test_sim_burst_paths.py checks them against the compiled header): k_detect's tile, the LDS
# window of a tile (tile + forward halo) and the length of a wavefront's pending list
TILE, WWIN, MAX_PEND = 1024, 1024 + 256, 8
THR_LSB2 = 400.0                    # threshold: 20 LSB, between the noise (+-2 LSB) and the carrier (>= 27 LSB)
CARRIER = 30                        # carrier: 27 .. 33 LSB, |IQ|^2 below half of a preamble chip's (>= 95 LSB)
RATES = (2, 4, 6, 8, 12, 20)        # samples per symbol


def _noise(rng, n):
    return rng.integers(-2, 3, n).astype(np.int64), rng.integers(-2, 3, n).astype(np.int64)


def _put_burst(i, q, rng, p, sps, bits, ties=(), amp=(50, 100)):
    """A preamble with chip 0 at p (chips 0, 2, 7, 9: 95 - 105 LSB) and the PPM bits after it: the high chip of bit k is
    set to 50 - 100 LSB.  Bits in `ties` get no pulse, and their two tap samples (demod.py:87-92) are made equal: x1 == x0."""
    half = sps // 2
    n = len(i)
    for c in (0, 2, 7, 9):
        s = p + c * half
        i[s:min(n, s + half)] = rng.integers(95, 106)
    for k, b in enumerate(bits):
        j1 = p + 8 * sps + k * sps
        if j1 + half >= n:
            break
        if k in ties:
            i[j1 + half], q[j1 + half] = i[j1], q[j1]
            continue
        s = j1 if b else j1 + half
        i[s:min(n, s + half)] = rng.integers(amp[0], amp[1] + 1)


def _fall_below(i, q, fall):
    """the run falls at `fall` even where a data chip of its burst lies there"""
    if fall < len(i):
        i[fall], q[fall] = 0, 0


def _frame(rng):
    return M.make_frame(17, rng)


def long_pulses(sps, seed=0):
    """One stream of long-pulse bursts, each in its own three tiles (local index == stream offset in a canonical call, so
    tiles start at multiples of TILE).  Returns (i, q, cases): cases = [(name, p, route)], route "long" (the run leaves
    the LDS window of its rise tile: k_longrun) or "window" (it does not: k_detect).

      rise at the tile's last samples with runs of WWIN - r - 1, WWIN - r, WWIN - r + 1 (r = rise - tile start): on both
      sides of the point where k_longrun takes over; runs over several tiles; ties x1 == x0 inside and after the run."""
    rng = np.random.default_rng(1000 * sps + seed)
    specs = []
    for r in (1023, 1017, 990):
        for d in (-1, 0, 1):
            specs.append(("r=%d run=WWIN-r%+d" % (r, d), r, WWIN - r + d))
    specs += [("run over 3 tiles", 300, 3 * TILE + 77), ("run over 5 tiles", 611, 5 * TILE + 400)]
    burst = 120 * sps
    n = 0
    slots = []
    for name, r, L in specs:
        t0 = (n // TILE + 2) * TILE
        slots.append((name, t0 + r, L))
        n = t0 + r + max(L, L // 2 + burst) + 3 * TILE
    i, q = _noise(rng, n)
    cases = []
    for name, rise, L in slots:
        fall = rise + L
        p = (rise + fall) // 2
        i[rise:fall] = CARRIER + rng.integers(-3, 4, L)
        ties = set(int(v) for v in rng.choice(112, 12, replace=False))
        _put_burst(i, q, rng, p, sps, _frame(rng), ties=ties)
        _fall_below(i, q, fall)
        t0 = rise - rise % TILE
        cases.append((name, p, "long" if fall >= t0 + WWIN else "window"))
    return i, q, cases


def long_pulse_at_end(sps, kind, seed=0):
    """A long pulse at the end of a stream of 8 tiles (+ a few samples).  kind:
      "straddles"  the burst runs past the end of the call: no PDU (dem false, demod.py:82), the clipped branch
      "fall last"  the run falls on the call's last scanned sample (in0 index N - 1: stream offset n - 8 sps)
      "high at end" the run is still high on the last scanned sample: no fall, no pulse (framer.py:102-108)
    Returns (i, q, p or None)."""
    rng = np.random.default_rng(7000 + 10 * sps + len(kind) + seed)
    H = 8 * sps
    rise = 7 * TILE + 1000
    if kind == "straddles":                 # centre within 119.5 sps of the end, fall before the scan's end
        L = 2 * 111 * sps - 10
        n = rise + L + 3 + H
    else:
        L = WWIN + 40
        n = rise + L + (H if kind == "fall last" else 0)
    i, q = _noise(rng, n)
    # a regular burst early on, so that the stream has a record through the ordinary route too
    _put_burst(i, q, rng, 700, sps, _frame(rng))
    fall = rise + L
    i[rise:fall] = CARRIER + rng.integers(-3, 4, fall - rise)
    p = (rise + fall) // 2
    _put_burst(i, q, rng, p, sps, _frame(rng), ties={3, 50, 100})
    _fall_below(i, q, fall)
    assert fall >= rise - rise % TILE + WWIN
    if kind == "straddles":
        assert p + 119 * sps + sps // 2 >= n and fall < n - (H - 1)
    elif kind == "fall last":
        assert fall == n - H                # in0 index N - 1 (the history holds H - 1 samples)
    return i, q, (None if kind == "high at end" else p)


def signed_zero_runs(sps, seed=0):
    """|IQ|^2 floats for thr 0.0: a negative floor, runs of +0.0 / -0.0 / small positive samples (all >= 0.0: above the
    threshold) with long-pulse bursts on them -- noise windows of mixed signed zeros (a zero median is +0.0), bit pairs
    +0/-0, -0/+0, +0/+0 (ties: bit 0) -- some runs short enough for k_detect, most leaving the LDS window.  Returns (x, ps)."""
    rng = np.random.default_rng(500 + sps + seed)
    burst = 120 * sps
    specs = [(1023, WWIN - 1023), (1000, WWIN - 1000 - 1), (200, 3 * TILE), (900, WWIN - 900 + 1), (50, 2 * TILE + 5)]
    n = sum(3 * TILE + max(L, L // 2 + burst) for _, L in specs) + 4 * TILE
    x = -(np.float32(0.25) + rng.random(n, dtype=np.float32))
    ps = []
    pos = TILE
    half = sps // 2
    for r, L in specs:
        t0 = (pos // TILE + 1) * TILE
        rise, fall = t0 + r, t0 + r + L
        u = rng.random(L)
        x[rise:fall] = np.where(u < 0.35, np.float32(-0.0), np.where(u < 0.7, np.float32(0.0),
                                                                     (rng.random(L) * 0.01).astype(np.float32)))
        p = (rise + fall) // 2
        for c in (0, 2, 7, 9):
            x[p + c * half:p + c * half + half] = np.float32(1.0)
        for c in (1, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15):
            if p + c * half + half <= fall:
                x[p + c * half:p + c * half + half] = np.float32(0.0) if c % 2 else np.float32(-0.0)
        bits = _frame(rng)
        for k, b in enumerate(bits):
            j1 = p + 8 * sps + k * sps
            if k % 9 == 4:                                        # a tie of signed zeros, three sign patterns
                x[j1], x[j1 + half] = [(np.float32(0.0), np.float32(-0.0)), (np.float32(-0.0), np.float32(0.0)),
                                       (np.float32(0.0), np.float32(0.0))][k % 3]
                continue
            s = j1 if b else j1 + half
            x[s:s + half] = np.float32(0.5) + np.float32(0.5) * rng.random(dtype=np.float32)
        x[fall] = np.float32(-0.5)                                # the run falls there, whatever bit lies on it
        ps.append(p)
        pos = p + max(L // 2, burst) + TILE
    assert pos < n
    return x[:pos + TILE].copy(), ps


def preamble_train(sps, n_tiles=32, seed=0, garble=True):
    """Bare preambles 8 - 12 symbols apart (chip 0 at 60 - 105 LSB; every one a matched centre, most inside the previous
    kept one's 63-symbol gate) in stretches of a few tiles, separated by quiet, plus DF17 replies on top of parts of the
    train (garble).  At sps >= 6 more than MAX_PEND bursts wait for their samples in one tile (pending_routes).  At 4 Msps a
burst waits only if its centre lies in the last 222 samples of its tile, at most 7 separate preambles (8 symbols apart):
chained_preambles() fills the list there.  At 2 Msps no centre of a tile's own samples waits at all (p + 239 < WWIN), so
no list fills.  Returns (i, q)."""
    rng = np.random.default_rng(3000 + sps + seed)
    n = n_tiles * TILE + 517
    i, q = _noise(rng, n)
    half = sps // 2
    pos = 150
    while pos < n - 16 * half:
        stretch_end = min(n - 16 * half, pos + int(rng.integers(3, 7)) * TILE)
        gap = int(rng.choice((8, 8, 8, 9, 10, 12)))              # symbols between preambles, one spacing per stretch
        while pos < stretch_end:
            a = int(rng.integers(60, 106))
            for c in (0, 2, 7, 9):
                i[pos + c * half:pos + c * half + half] = a
            pos += gap * sps
        pos += int(rng.integers(1, 3)) * TILE // 2 + int(rng.integers(0, 100))
    if garble:
        for s in rng.integers(0, n - 130 * sps, max(2, n_tiles // 4)):
            bits = _frame(rng)
            env = M.burst_waveform(bits, sps)
            e = min(n, s + len(env))
            on = env[:e - s] > 0
            i[s:e][on] += int(rng.integers(40, 90))
    return i, q


def pending_routes(cands, sps, chunk=None):
    """The pending-list routes of k_detect for these matched centres (stream offsets of a canonical call: local index ==
    stream offset, tiles at multiples of TILE).  A centre of tile t0 whose last bit pair (p + 119 sps + sps/2) lies past
    t0 + WWIN waits on its wavefront's list until a later window holds that pair (pend_step); with MAX_PEND waiting it is
    sliced from global memory at once (burst_from_window).  chunk: samples per wavefront (a multiple of TILE, as
    adsb_plan.h's plan_chunks makes it; None = one wavefront for the whole stream): the list starts empty with every chunk
    and whatever still waits at a chunk's last tile is finished by pend_flush.
    Returns (full, flushed_full): the centres sliced because the list was full, and those flushed from a list that was
    still full at its chunk's end."""
    half = sps // 2
    cands = np.asarray(cands, dtype=np.int64)
    pend, full, flushed = [], [], []
    end = int(cands.max()) + TILE if len(cands) else 0
    for t0 in range(0, end, TILE):
        if chunk and t0 % chunk == 0:
            pend = []
        pend = [(c, e) for c, e in pend if e >= t0 + WWIN]
        for p in cands[(cands >= t0) & (cands < t0 + TILE)]:
            e = int(p) + 119 * sps + half
            if e < t0 + WWIN:
                continue
            if len(pend) < MAX_PEND:
                pend.append((int(p), e))
            else:
                full.append(int(p))
        if chunk and (t0 + TILE) % chunk == 0:
            if len(pend) == MAX_PEND:
                flushed += [c for c, _ in pend]
            pend = []
    return np.array(full, dtype=np.int64), np.array(flushed, dtype=np.int64)


def full_list_centres(cands, sps):
    """pending_routes(cands, sps)[0]: one wavefront over the whole stream"""
    return pending_routes(cands, sps)[0]


def chained_preambles(sps, seed=0):
    """Preambles 7 chips apart, each 0.64 times as strong as the one before it (|IQ|^2; 0.8 in amplitude): chip 7 of one is
    chip 0 of the next, its chip 9 is the next one's chip 2, and its chip 14 -- which must stay low -- is chip 0 of the one
    after that, at 0.41 of its own level, below half.  So matched centres are 3.5 symbols apart, twice as dense as
    separate preambles allow, and at 4 Msps more than MAX_PEND of them wait in one tile.

    In each of a few tiles: a bare preamble at K (window route, kept), a chain of eight whose centres lie where a burst waits for
    later samples (the first past WWIN - 119.5 sps) but inside K's gate (K + 63 sps: gated out), and a DF17 burst just past
    the gate: the list is full when it arrives, and the gate keeps it.  sps 4, 6 and 8 (at 12 and 20 Msps every centre
    waits, and the trains fill the lists).  Returns (i, q, kept): kept = the DF17 bursts' centres."""
    assert sps in (4, 6, 8)
    rng = np.random.default_rng(6000 + sps + seed)
    half = sps // 2
    p0 = WWIN - (119 * sps + half)                  # first centre of a tile whose burst waits
    amps = (127, 102, 81, 65, 52, 42, 33, 27)
    n = 14 * TILE
    i, q = _noise(rng, n)
    kept = []
    for t0 in (2 * TILE, 6 * TILE, 10 * TILE):
        s = t0 + p0 + int(rng.integers(1, 6))
        c7 = s + 7 * 7 * half
        K = c7 - 63 * sps + int(rng.integers(0, 4))         # the chain lies inside K's gate
        assert K + 16 * half < s and K >= t0
        _put_burst(i, q, rng, K, sps, [])                  # a bare preamble: its bits would lie on the chain
        for k, a in enumerate(amps + (21,)):                # in order: a later preamble's pulse overwrites a shared chip
            for c in ((0, 2, 7, 9) if k < len(amps) else (0, 2)):   # (the last two pulses keep chip 14 of the 7th low)
                j = s + 7 * k * half + c * half
                i[j:j + half] = a
        c9 = max(K + 63 * sps + 1, c7 + 16 * half) + int(rng.integers(0, 4))
        assert c9 < t0 + TILE
        _put_burst(i, q, rng, c9, sps, _frame(rng))
        kept.append(c9 + half // 2)                         # the centre of its chip-0 pulse
    return i, q, kept


def matched_centres(x, sps, thr):
    """every matched centre of a canonical call (framer.py:113,137-147), stream offsets"""
    H = 8 * sps
    buf = np.concatenate([np.zeros(H - 1, np.float32), np.asarray(x, np.float32)])
    with np.errstate(all="ignore"):
        c, _ = O.pulses_of_call(buf, len(x), np.float32(thr), np.float32(0.0))
        c = c[c + 15 * (sps // 2) < len(buf)]
        c = c[O.match_preamble(buf, c, sps)] if len(c) else c
    return c - (H - 1)


def streams(sps):
    """(name, i, q, routes): every integer-component stream of one rate, with the routes (simlib.ROUTES) at least one KEPT
    record of it must have been built by, in a canonical call"""
    i, q, cases = long_pulses(sps)
    assert any(r == "long" for _, _, r in cases) and any(r == "window" for _, _, r in cases)
    yield "long pulses", i, q, {"long_fast"}
    for kind in ("straddles", "fall last", "high at end"):
        i, q, p = long_pulse_at_end(sps, kind)
        clipped = kind == "straddles" or (p is not None and p + 136 * sps >= len(i))
        yield "long pulse, " + kind, i, q, (set() if p is None else {"long_clipped" if clipped else "long_fast"})
    i, q = preamble_train(sps)
    yield "preamble train", i, q, ({"pend_full", "flush"} if sps >= 6 else {"flush"} if sps == 4 else set())
    if sps in (4, 6, 8):
        i, q, _ = chained_preambles(sps)
        yield "chained preambles", i, q, {"pend_full"}


def threshold(fmt, scale):
    """THR_LSB2 in the format's |IQ|^2 at this scale (edge_cases.unit2), float32"""
    import edge_cases as E
    return np.float32(THR_LSB2 * E.unit2(fmt, scale))


def slice_cases(sps, seed=0):
    """k_slice (the stand-alone demod, demod.py:57-136) at its edges: (name, in0, tag_idx) with tag_idx local to in0.
      * the last tag that is sliced (p + 119 sps + sps/2 == n - 1) and the first that is dropped (== n)
      * tags in front of the chunk (negative), duplicates, unsorted
      * 0/0, x/0, inf/inf, subnormal/normal ratios
      * more than 8192 tags (the library's k_slice grid is 2048 workgroups of four wavefronts)"""
    rng = np.random.default_rng(900 + sps + seed)
    half = sps // 2
    n = 40 * 120 * sps + 1000
    x = (rng.random(n, dtype=np.float32) * np.float32(0.01)).astype(np.float32)
    special = np.array([0.0, 0.0, 1.0, 0.0, np.inf, np.inf, 1e-40, 1.0, 3e-45, 2.0, np.nan, 1.0, 0.0, -0.0], np.float32)
    for s in range(50, n - 120 * sps, 977):
        for k in range(0, 112, 3):
            j1 = s + 8 * sps + k * sps
            m = (k // 3) % (len(special) // 2)
            x[j1], x[j1 + half] = special[2 * m], special[2 * m + 1]
    last = n - 1 - (119 * sps + half)                   # p + 119 sps + half == n - 1: sliced; one more: dropped
    base = np.arange(50, n - 120 * sps, 977, dtype=np.int64)
    yield "edges", x, np.array([last, last + 1, last - 1, 0, -1, -8 * sps, -10 ** 6, n - 1, n, 10 ** 9], np.int64)
    yield "duplicates unsorted", x, np.concatenate([base[::-1], base[:3], [last + 1, last, last]]).astype(np.int64)
    many = rng.integers(-200, n, 9000).astype(np.int64)
    many[::7] = last
    many[1::7] = last + 1
    yield "9000 tags", x, many


def fixture_stream(sps):
    """|IQ|^2 floats of the reference fixtures (tools/make_golden_paths.py): the long pulses, a train and a long pulse whose
    burst straddles the end, back to back; and the threshold"""
    import edge_cases as E
    i1, q1, _ = long_pulses(sps)
    i2, q2 = preamble_train(sps, n_tiles=16)
    i3, q3, _ = long_pulse_at_end(sps, "straddles")
    _, x = E.encode("mag2", np.r_[i1, i2, i3], np.r_[q1, q2, q3], None)
    return x, threshold("mag2", None)
