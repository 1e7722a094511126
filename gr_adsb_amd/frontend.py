"""Whole-buffer and sharded front end over the C ABI: the bulk (bench) path.

FrontEnd.process_* == one canonical framer.work() + demod.work() over a buffer (SURVEY.md §8a chunk
semantics); shard_plan/process_shard/stitch tile a long stream across GPUs as independent overlapped
time shards whose candidate lists are stitched on the host -- no collective.
"""
import numpy as np

from . import _native

NOISE_BACK = 100          # framer.py:31 look-back for the SNR median


def shard_plan(stream_len, n_shards, sps, max_run=256, align=4096):
    """Split [0, stream_len) into n_shards owner ranges with the halos each one needs:
    back = 100 (noise median) + 1, forward = max_run (longest pulse followed) + 120*sps (preamble +
    112 bits).  Returns a list of dicts(own_lo, own_hi, lo, hi) in stream offsets; buffer starts are
    aligned down to 4 samples (16-byte loads)."""
    per = -(-stream_len // n_shards)
    per = -(-per // align) * align
    plans = []
    for g in range(n_shards):
        own_lo = min(stream_len, g * per)
        own_hi = min(stream_len, (g + 1) * per)
        lo = max(0, own_lo - (NOISE_BACK + 8 * sps + 4))
        lo -= lo % 4
        hi = min(stream_len, own_hi + max_run + 121 * sps)
        plans.append(dict(own_lo=own_lo, own_hi=own_hi, lo=lo, hi=hi))
    return plans


def _after_torch(ctx, t):
    """The context runs on its own HIP streams: whatever torch still has queued on ITS current stream for this tensor
    (the kernels that produce it) must have finished before our kernels read it.  A device-side dependency -- an event
    recorded on torch's stream that the context's streams wait for (adsb_wait_for_event); the host does not block, so
    a producer still running does not serialise the submit / wait pipeline.
    (adsb_set_stream / FrontEnd.use_torch_stream is the alternative: share torch's stream and skip this.)"""
    import torch
    assert t.is_cuda and t.is_contiguous()
    # a ring of eight re-recordable events per context: the wait is queued with the NEXT call on the context (which follows
    # at once), so an event is long done with by the time its turn comes again -- and none is created per call
    ring = getattr(ctx, "_torch_events", None)
    if ring is None:
        ring = ctx._torch_events = [[torch.cuda.Event() for _ in range(8)], 0]
    ev = ring[0][ring[1] & 7]
    ring[1] += 1
    ev.record(torch.cuda.current_stream(t.device))
    ctx.wait_for_event(ev.cuda_event)


class FrontEnd:
    def __init__(self, fs, threshold, device=0, timing=False, flags=0):
        self.fs = float(fs)
        self.sps = int(fs // 1e6)
        self.ctx = _native.Context(fs, threshold, device=device, flags=int(flags) | (_native.FLAG_TIMING if timing else 0))

    def set_threshold(self, thr):
        self.ctx.set_threshold(thr)

    def use_torch_stream(self, stream):
        self.ctx.set_stream(stream.cuda_stream)

    # -- host buffers -------------------------------------------------------------------------------
    def process_iq(self, iq, abs_offset=0):
        return self.ctx.process_iq(iq, abs_offset)

    def process_mag2(self, x, abs_offset=0):
        return self.ctx.process_mag2(x, abs_offset)

    def process_iq16(self, iq16, abs_offset=0, scale=None):
        """iq16: interleaved int16 I,Q; scale: float32 multiplier per component (default 1/32768)."""
        if scale is not None:
            self.ctx.set_iq16_scale(scale)
        return self.ctx.process_iq16(iq16, abs_offset)

    def process_iq8(self, iq8, abs_offset=0, scale=None):
        """iq8: interleaved 8-bit I,Q: int8 (cs8) or uint8 (cu8, offset binary around 127.5: RTL-SDR), chosen by
        the array's dtype; scale: float32 multiplier per component (defaults 1/128 resp. 1/255 per half LSB)."""
        iq8 = np.asarray(iq8)
        fmt = _native.FMT_CU8 if iq8.dtype == np.uint8 else _native.FMT_SC8
        if scale is not None:
            self.ctx.set_format_scale(fmt, scale)
        return self.ctx.process_format(fmt, iq8, abs_offset)

    def process_format(self, fmt, data, abs_offset=0):
        return self.ctx.process_format(fmt, data, abs_offset)

    # -- torch tensors already in HBM ---------------------------------------------------------------
    def process_format_tensor(self, fmt, t, abs_offset=0, fetch=True):
        """t: contiguous CUDA tensor whose first dimension is the sample count ([n,2] for the IQ formats)."""
        _after_torch(self.ctx, t)
        return self.ctx.process_format_device(fmt, t.data_ptr(), t.shape[0], abs_offset, fetch=fetch)

    def submit_format_tensor(self, fmt, t, abs_offset=0):
        _after_torch(self.ctx, t)
        return self.ctx.submit_format_device(fmt, t.data_ptr(), t.shape[0], abs_offset)

    def process_iq_tensor(self, t, abs_offset=0, fetch=True):
        """t: float32 [n,2] (or complex64 [n]) CUDA tensor, contiguous."""
        _after_torch(self.ctx, t)
        n = t.shape[0]
        return self.ctx.process_iq_device(t.data_ptr(), n, abs_offset, fetch=fetch)

    def process_mag2_tensor(self, t, abs_offset=0, fetch=True):
        _after_torch(self.ctx, t)
        return self.ctx.process_mag2_device(t.data_ptr(), t.shape[0], abs_offset, fetch=fetch)

    def submit_iq16_tensor(self, t, abs_offset=0):
        """t: int16 [n,2] CUDA tensor (interleaved I,Q)."""
        _after_torch(self.ctx, t)
        return self.ctx.submit_iq16_device(t.data_ptr(), t.shape[0], abs_offset)

    def submit_iq_tensor(self, t, abs_offset=0):
        """Queue a canonical pass over t (up to _native.MAX_IN_FLIGHT in flight); returns a ticket for wait()."""
        _after_torch(self.ctx, t)
        return self.ctx.submit_iq_device(t.data_ptr(), t.shape[0], abs_offset)

    def submit_shard_tensor(self, t, origin, own_lo, own_hi, stream_len, fmt=0, head_cands=0):
        _after_torch(self.ctx, t)
        return self.ctx.submit_shard_device(fmt, t.data_ptr(), t.shape[0], origin, own_lo, own_hi, stream_len, head_cands)

    def process_sharded_tensor(self, fmt, t, shards, abs_offset=0, out=None):
        """t as `shards` overlapped time shards on this GPU, pipelined and stitched in C (adsb_process_sharded_device):
        bit-identical to process_format_tensor over the whole tensor."""
        _after_torch(self.ctx, t)
        return self.ctx.process_sharded_device(fmt, t.data_ptr(), t.shape[0], shards, abs_offset, out=out)

    def wait(self, ticket, fetch=True, copy=True):
        return self.ctx.wait(ticket, fetch=fetch, copy=copy)

    # -- many receivers, one GPU: a batch of independent streams in one device pass -------------------
    def process_batch(self, fmt, arrays, thresholds=None, abs_offsets=None):
        """arrays[i]: host array of item i in the format's layout -> (records, item_first); item i's records, those of
        process_format(fmt, arrays[i]) at thresholds[i], are records[item_first[i]:item_first[i+1]] (Context.process_batch).
        On a FLAG_FEC_SOFT_BATCH context the records are soft-repaired, each against its own item's samples, and
        ctx.last_batch_soft() holds their SOFT_DTYPE rows, row t for records[t]."""
        return self.ctx.process_batch(fmt, arrays, thresholds, abs_offsets)

    def process_batch_tensors(self, fmt, tensors, thresholds=None, abs_offsets=None):
        """The same for contiguous CUDA tensors (first dimension = samples; views into one allocation are fine as long as each
        starts on a 16-byte boundary).  One event for the call: the tensors are all on torch's current stream."""
        tensors = list(tensors)
        if tensors:
            for t in tensors:
                assert t.is_cuda and t.is_contiguous()
            _after_torch(self.ctx, tensors[0])
        return self.ctx.process_batch_device(fmt, [t.data_ptr() for t in tensors], [t.shape[0] for t in tensors],
                                             thresholds, abs_offsets)

    @property
    def last_batch_fallbacks(self):
        return self.ctx.last_batch_fallbacks

    # -- many receivers that go on: streams carried across batch calls -----------------------------------
    def receivers(self, n, fmt=None, starts=None, msg_filter=None, ages=False, shared=False, dedup=False, positions=None, soft_fec=False):
        """n receiver streams on this context (Receivers below).  fmt: one of _native.FMT_*, or None: by the arrays' dtype.
        starts / msg_filter: FLAG_STREAM_DECODE contexts, the streams' start timestamps and their decoders' msg_filter.
        ages: the context also has FLAG_PLANE_AGES (ValueError otherwise): .planes(seen=True) and .expire(cutoffs).
        shared: the context also has FLAG_STREAM_DECODE_SHARED (ValueError otherwise): ONE decoder behind all n streams.
        dedup: True, or (window_s, horizon_s): the context also has FLAG_STREAM_DEDUP (ValueError otherwise).
        positions: [(lat_deg, lon_deg, alt_m), ...], the antennas of streams 0, 1, ... on the WGS-84 ellipsoid (None in the
        list: that stream has none); needs dedup (ValueError otherwise): Receivers.mlat().
        soft_fec: True, or a dict of rule fields (n_weak, max_flips, min_key): the context also has FLAG_FEC_SOFT_BATCH (ValueError
        otherwise): every push repairs each stream's parity failures from that stream's own samples; Receivers.soft."""
        return Receivers(self.ctx, n, fmt, starts, msg_filter, ages, shared, dedup, positions, soft_fec)

    def shard_tensor(self, t, origin, own_lo, own_hi, stream_len, fmt=0, head_cands=0):
        _after_torch(self.ctx, t)
        return self.ctx.shard_device(fmt, t.data_ptr(), t.shape[0], origin, own_lo, own_hi, stream_len, head_cands)

    def stitch(self, cand_lists):
        c = np.concatenate([np.asarray(x, dtype=_native.BURST_DTYPE) for x in cand_lists]) if len(cand_lists) else \
            np.zeros(0, dtype=_native.BURST_DTYPE)
        return _native.stitch(c, self.sps)

    def stats(self):
        return self.ctx.stats()

    @staticmethod
    def snr(bursts):
        return _native.snr_db(bursts["peak"], bursts["median"])

    @staticmethod
    def bits(bursts):
        return _native.unpack_bits(bursts["bits"])[:, :112]


_FMT_OF_DTYPE = {np.dtype(dt): fmt for fmt, (dt, _) in _native.FMT_LAYOUT.items()}


class Receivers:
    """A fleet of receivers on one context (FrontEnd.receivers): every push() runs the next chunk of any subset of the streams
    through one device pass (adsb_process_stream_batch), seam-exact: a stream's records over all pushes and its finish() are
    those of process_format over the concatenation of its chunks, delayed by the look-ahead of 256 + 121 * sps samples.
    .overlong counts, over all streams, what the bounded carry made it leave out (pulses still high at the end of a call's
    buffer).  One set of streams per context; close() releases it.
    On a FLAG_STREAM_DECODE context every stream has a decoder of its own: after push() / finish(), .rows holds the list of
    DECODED_DTYPE row arrays that matches the returned record arrays (row t of a stream belongs to its record t;
    _native.decoded_pdu turns a row into the reference's published PDU).  starts: the streams' start timestamps (a record's
    PDU timestamp is start + offset / fs), msg_filter: "All Messages" (default) or "Extended Squitter Only".
    shared (a FLAG_STREAM_DECODE | FLAG_STREAM_DECODE_SHARED context): ONE decoder behind all streams, fed every push's records
    in the order ascending (timestamp, position in the push's list), so `starts` have to be real, comparable times.  .rows is
    as above -- each row what the one decoder made of that record --, .order holds the publication order of the last push /
    finish as positions in the concatenation of the returned record arrays, and planes(), merged(), table() and expire()
    address the one plane table: planes() returns ONE row array (seen=True: one (rows, last_seen) pair), expire() takes one
    cutoff, and none of them takes ids.  The same reply heard by several receivers counts once per hearing,
    unless dedup (a context that also has FLAG_STREAM_DEDUP; True, or (window_s, horizon_s) for other than 0.002 s and 1.0 s):
    then it is published once, the other hearings' rows have port DEC_DUPLICATE, and .duplicates holds, beside .order, -1 /
    -2 (the match lies in an earlier push) / the position of the earliest-published match of the last push or finish.
    positions (with dedup): the antennas' (lat_deg, lon_deg, alt_m); mlat() then locates the replies that four or more
    positioned receivers heard, from their arrival times alone (include/adsb_hip.h MULTILATERATION: pass `starts` relative to
    a session epoch, not Unix times, or the double's spacing costs 71 m).
    soft_fec (a context that also has FLAG_FEC_SOFT_BATCH; True, or a dict of rule fields for other than 8 / 3 / 0.0): the
    soft-decision CRC repair (include/adsb_hip.h SOFT REPAIR, IN A BATCH) runs in every push, each stream's records against its
    own samples, before the decoders, the de-duplication and mlat() see them; after push() / finish(), .soft holds the list of
    SOFT_DTYPE row arrays that matches the returned record arrays (nflip != 0: repaired by the soft rule)."""

    def __init__(self, ctx, n, fmt=None, starts=None, msg_filter=None, ages=False, shared=False, dedup=False, positions=None,
                 soft_fec=False):
        self.ctx, self.n, self.fmt = ctx, int(n), fmt
        self.decode = bool(getattr(ctx, "flags", 0) & _native.FLAG_STREAM_DECODE)
        self.ages = bool(ages)
        self.shared = bool(shared)
        self.rows = []
        self.order = np.zeros(0, dtype=np.int32)
        self.dedup = dedup is not False and dedup is not None
        self.duplicates = np.zeros(0, dtype=np.int32)
        self.soft = []
        if soft_fec is not False and soft_fec is not True and not isinstance(soft_fec, dict):
            raise ValueError("soft_fec: True, or a dict of rule fields")
        self.soft_fec = None if soft_fec is False else dict(_native.SOFT_FEC_DEFAULTS, **({} if soft_fec is True else soft_fec))
        if self.soft_fec is not None and set(self.soft_fec) != set(_native.SOFT_FEC_DEFAULTS):
            raise ValueError("soft_fec: the rule's fields are n_weak, max_flips, min_key")
        if (self.soft_fec is not None) != bool(getattr(ctx, "flags", 0) & _native.FLAG_FEC_SOFT_BATCH):
            raise ValueError("soft_fec needs, and its absence excludes, a FLAG_FEC_SOFT_BATCH context")
        if self.dedup != bool(getattr(ctx, "flags", 0) & _native.FLAG_STREAM_DEDUP):
            raise ValueError("dedup needs, and its absence excludes, a FLAG_STREAM_DEDUP context")
        if positions is not None and not self.dedup:
            raise ValueError("positions need dedup: multilateration reads the de-duplication carry")
        if positions is not None and len(positions) > self.n:
            raise ValueError("more positions than streams")
        if self.shared != bool(getattr(ctx, "flags", 0) & _native.FLAG_STREAM_DECODE_SHARED):
            raise ValueError("shared=True needs, and shared=False excludes, a FLAG_STREAM_DECODE | FLAG_STREAM_DECODE_SHARED context")
        if self.ages and not (self.decode and getattr(ctx, "flags", 0) & _native.FLAG_PLANE_AGES):
            raise ValueError("ages needs a FLAG_STREAM_DECODE | FLAG_PLANE_AGES context")
        if not self.decode and (starts is not None or msg_filter is not None):      # (before any stream is opened)
            raise ValueError("starts / msg_filter need a FLAG_STREAM_DECODE context")
        ctx.open_streams(self.n)
        if self.soft_fec is not None and soft_fec is not True:
            ctx.set_soft_fec(**self.soft_fec)
        if self.decode:
            if msg_filter is not None:
                ctx.set_streams_decoder(msg_filter)
            for i, t in enumerate(starts if starts is not None else []):
                ctx.set_stream_start(i, t)
        if self.dedup and dedup is not True:
            ctx.set_streams_dedup(*dedup)
        for i, pos in enumerate(positions if positions is not None else []):
            if pos is not None:
                ctx.set_stream_ecef(i, *_native.geodetic_to_ecef(*pos))

    def _run(self, arrays, ids, thresholds, end):
        ids = list(range(len(arrays))) if ids is None else [int(i) for i in ids]
        assert len(ids) == len(arrays)
        if not ids:
            self.rows = []
            self.order = np.zeros(0, dtype=np.int32)
            self.duplicates = np.zeros(0, dtype=np.int32)
            self.soft = []
            return []
        arrays = [np.asarray(a) for a in arrays]
        fmt = self._last_fmt = self.fmt if self.fmt is not None else _FMT_OF_DTYPE[arrays[0].dtype]
        recs, first = self.ctx.process_stream_batch(fmt, ids, arrays, thresholds, end)
        if self.decode:
            rows = self.ctx.last_stream_decoded()
            self.rows = [rows[first[i]:first[i + 1]] for i in range(len(ids))]
        if self.soft_fec is not None:
            soft = self.ctx.last_batch_soft()
            self.soft = [soft[first[i]:first[i + 1]] for i in range(len(ids))]
        if self.shared:
            self.order = self.ctx.last_stream_order()
        if self.dedup:
            self.duplicates = self.ctx.last_stream_duplicates()
        return [recs[first[i]:first[i + 1]] for i in range(len(ids))]

    def push(self, arrays, ids=None, thresholds=None):
        """arrays[i]: the next samples of stream ids[i] (None: streams 0 .. len(arrays) - 1), any length -> a list of record
        arrays, one per pushed stream"""
        return self._run(arrays, ids, thresholds, False)

    def finish(self, ids=None, thresholds=None):
        """End streams `ids` (None: all): what they still owe, with the end-of-call rules -> a list of record arrays.  The
        streams are fresh afterwards."""
        ids = list(range(self.n)) if ids is None else list(ids)
        live = [i for i in ids if self.ctx.stream_state(i)[0] > 0]
        dt = _native.FMT_LAYOUT[self.fmt][0] if self.fmt is not None else None
        out = {i: np.zeros(0, dtype=_native.BURST_DTYPE) for i in ids}
        if live:
            if dt is None:
                dt = _native.FMT_LAYOUT[self._last_fmt][0]
            thr = None if thresholds is None else [thresholds[ids.index(i)] for i in live]
            for i, r in zip(live, self._run([np.zeros(0, dtype=dt)] * len(live), live, thr, True)):
                out[i] = r
        if self.decode:
            rows = dict(zip(live, self.rows)) if live else {}
            self.rows = [rows.get(i, np.zeros(0, dtype=_native.DECODED_DTYPE)) for i in ids]
        if self.soft_fec is not None:
            soft = dict(zip(live, self.soft)) if live else {}
            self.soft = [soft.get(i, np.zeros(0, dtype=_native.SOFT_DTYPE)) for i in ids]
        return [out[i] for i in ids]

    def planes(self, ids=None, seen=False):
        """FLAG_STREAM_DECODE contexts: what each receiver sees now -- a list of DECODED_DTYPE row arrays, one per stream of
        `ids` (strictly ascending; None: every stream), each in ascending address order, from one device snapshot of the
        decoders' store (adsb_stream_planes; _native.plane_entry turns a row into the reference's plane_dict entry).
        seen (receivers(ages=True)): a list of (rows, last_seen) pairs, last_seen the int64 clocks of the rows."""
        if not self.decode:
            raise ValueError("planes() needs a FLAG_STREAM_DECODE context")
        if self.shared:                              # the one decoder's table: the store's stream 0
            if ids is not None:
                raise ValueError("a shared decoder has one table: planes() takes no ids")
            return self._per_stream_planes([0], seen)[0]
        return self._per_stream_planes(ids, seen)

    def _per_stream_planes(self, ids, seen):
        if seen:
            if not self.ages:
                raise ValueError("planes(seen=True) needs receivers(ages=True)")
            rows, ages, first = self.ctx.stream_planes(ids, seen=True)
            return [(rows[first[i]:first[i + 1]], ages[first[i]:first[i + 1]]) for i in range(len(first) - 1)]
        rows, first = self.ctx.stream_planes(ids)
        return [rows[first[i]:first[i + 1]] for i in range(len(first) - 1)]

    def expire(self, cutoffs, ids=None):
        """receivers(ages=True): every stream of `ids` (strictly ascending; None: all) forgets its planes with
        last_seen < its cutoff, as `del plane_dict[key]` (adsb_stream_planes_expire) -> the number removed.  cutoffs: one per
        stream of `ids`, or a scalar for all of them (streams do not share a clock: a scalar suits equal start timestamps)."""
        if not self.ages:
            raise ValueError("expire() needs receivers(ages=True)")
        if self.shared:
            if ids is not None or np.ndim(cutoffs) != 0:
                raise ValueError("a shared decoder has one table: expire() takes one cutoff and no ids")
            return self.ctx.expire_stream_planes(np.array([int(cutoffs)], dtype=np.int64), [0])
        k = self.n if ids is None else len(ids)
        cut = np.full(k, int(cutoffs), dtype=np.int64) if np.ndim(cutoffs) == 0 else np.asarray(cutoffs, dtype=np.int64)
        return self.ctx.expire_stream_planes(cut, ids)

    def merged(self, ids=None, cutoff=None, mlat=False):
        """receivers(ages=True): ONE picture out of every receiver's -- (rows, info), one DECODED_DTYPE row per aircraft any
        stream of `ids` (strictly ascending; None: all) holds, in ascending address order, and its _native.MERGED_DTYPE entry
        (adsb_stream_planes_merged).  Callsign, altitude, velocity and position each come from the receiver that has the field
        and heard the aircraft last (info["src_*"]: which one); num_msgs is the sum, info["last_seen"] the latest clock.
        cutoff: entries with last_seen < cutoff are left out (None: none is); the streams' clocks have to be comparable, i.e.
        `starts` real times.  _native.plane_entry(row, last_seen) turns a row into the reference's plane_dict entry.
        mlat=True (receivers(dedup=...) too): -> (rows, info, track_of, tracks): tracks is tracks(min_fixes=1), and track_of[j]
        the index in it of rows[j]'s address (-1 where it has no track), found with np.searchsorted on the two address-ordered
        results.  Aircraft known to MLAT alone are in tracks only.  rows and info are what merged() without mlat returns."""
        if not (self.decode and self.ages):
            raise ValueError("merged() needs receivers(ages=True) on a FLAG_STREAM_DECODE | FLAG_PLANE_AGES context")
        if self.shared:
            if ids is not None:
                raise ValueError("a shared decoder has one table: merged() takes no ids")
            ids = [0]
        rows, info = self.ctx.merged_planes(ids, cutoff)
        if not mlat:
            return rows, info
        tracks = self.tracks(min_fixes=1)
        at = np.searchsorted(tracks["icao"], rows["icao"])
        hit = at < len(tracks)
        hit[hit] = tracks["icao"][at[hit]] == rows["icao"][hit]
        return rows, info, np.where(hit, at, -1).astype(np.int32), tracks

    def track(self, t_lo=None, t_hi=None, solver="damped", restart=True, altitude=False, alt_weight=1.0, min_rx=4, **track_rule):
        """receivers(dedup=..., positions=...): one update of the device-side store of per-aircraft MLAT tracks
        (adsb_stream_mlat_track; include/adsb_hip.h MLAT TRACKS) from the fixes mlat() with these arguments would return for
        [t_lo, t_hi) -- the fixes stay on the device -> the call's totals as a dict (fixes, eligible, unusable, stale, rejected,
        taken, started, tracks).  track_rule: alpha, beta, gate_m, max_speed_mps, max_gap_s, restart_after, max_rms_m, min_up_m
        over _native.MLAT_TRACK_DEFAULTS (0.3, 0.05, 2000, 350, 30, 3, 500, 0).  A fix no later than its track's last one is stale,
        so none is taken twice; a rejected fix is not remembered, so let successive calls' ranges adjoin (t_lo = the last
        call's t_hi) rather than overlap.  The store outlives the carry; tracks() reads it, expire_tracks() and
        reset_tracks() shrink it."""
        if not self.dedup:
            raise ValueError("track() needs receivers(dedup=...)")
        if solver not in ("gauss-newton", "damped"):
            raise ValueError("solver is 'gauss-newton' or 'damped'")
        lo, hi = -np.inf if t_lo is None else t_lo, np.inf if t_hi is None else t_hi
        if solver == "damped":
            rule = _native.MLAT_RULE(_native.MLAT_SOLVER_LM, (_native.MLAT_RESTART if restart else 0) | (_native.MLAT_ALTITUDE if altitude else 0),
                                     int(min_rx), 0, float(alt_weight))
        else:
            rule = _native.MLAT_RULE(_native.MLAT_SOLVER_GN, 0, int(min_rx), 0, 0.0)
        return self.ctx.stream_mlat_track(rule, _native.mlat_track_rule(**track_rule), lo, hi)

    def tracks(self, min_fixes=3, cutoff=None):
        """The tracks with n_fixes >= min_fixes and last_ts >= cutoff (None: all), in ascending icao (adsb_stream_mlat_tracks):
        _native.MLAT_TRACK_DTYPE's fields and, computed here in plain NumPy from the row: latitude / longitude (degrees) /
        altitude_m by ecef_to_geodetic(x, y, z), and speed_kt (horizontal), heading_deg (clockwise from north, [0, 360)) and
        vertical_rate_fpm from (vx, vy, vz) in the local east / north / up frame at that position."""
        if not self.dedup:
            raise ValueError("tracks() needs receivers(dedup=...)")
        rows = self.ctx.stream_mlat_tracks(min_fixes, -np.inf if cutoff is None else cutoff)
        extra = ("latitude", "longitude", "altitude_m", "speed_kt", "heading_deg", "vertical_rate_fpm")
        out = np.zeros(len(rows), dtype=np.dtype(_native.MLAT_TRACK_DTYPE.descr + [(name, "<f8") for name in extra]))
        for name in _native.MLAT_TRACK_DTYPE.names:
            out[name] = rows[name]
        for j, r in enumerate(rows):
            out["latitude"][j], out["longitude"][j], out["altitude_m"][j] = _native.ecef_to_geodetic(r["x"], r["y"], r["z"])
        la, lo = np.radians(out["latitude"]), np.radians(out["longitude"])
        east = -np.sin(lo) * rows["vx"] + np.cos(lo) * rows["vy"]
        north = -np.sin(la) * np.cos(lo) * rows["vx"] - np.sin(la) * np.sin(lo) * rows["vy"] + np.cos(la) * rows["vz"]
        up = np.cos(la) * np.cos(lo) * rows["vx"] + np.cos(la) * np.sin(lo) * rows["vy"] + np.sin(la) * rows["vz"]
        out["speed_kt"] = np.hypot(east, north) * (3600.0 / 1852.0)
        out["heading_deg"] = np.degrees(np.arctan2(east, north)) % 360.0
        out["vertical_rate_fpm"] = up * (60.0 / 0.3048)
        return out

    def expire_tracks(self, cutoff):
        """Forget the tracks with last_ts < cutoff (adsb_stream_mlat_tracks_expire) -> their number."""
        return self.ctx.expire_mlat_tracks(cutoff)

    def reset_tracks(self):
        """Forget every track (adsb_stream_mlat_tracks_reset)."""
        self.ctx.reset_mlat_tracks()

    def mlat(self, t_lo=None, t_hi=None, min_rx=4, solver="gauss-newton", restart=True, altitude=False, alt_weight=1.0):
        """receivers(dedup=..., positions=...): the replies of the carry (the last `horizon` seconds) that at least min_rx
        positioned receivers heard, each located from its arrival times (adsb_stream_mlat) -> (fixes, member_stream, member_ts):
        fixes has _native.MLAT_DTYPE's fields and latitude / longitude (degrees) / altitude_m, converted on the host; the
        hearings of fixes[j] are member_*[first : first + n_rx].  t_lo / t_hi: only replies whose first hearing has
        t_lo <= ts < t_hi; None leaves that side open.  Read status (MLAT_OK), rms_m and n_rx before trusting a row.
        solver="damped": THE DAMPED RULE of include/adsb_hip.h (adsb_stream_mlat_rule) -- restart: a second run where the first
        fails or ends below the receivers; altitude: the reply's own altitude as one more row of weight alt_weight (metres of
        range per metre of height), which also allows min_rx=3 -- and fixes gains alt_ft, up_m, tries and aux_flags
        (_native.MLAT_AUX_*).  The other arguments are read with solver="damped" only."""
        if not self.dedup:
            raise ValueError("mlat() needs receivers(dedup=...)")
        if solver not in ("gauss-newton", "damped"):
            raise ValueError("solver is 'gauss-newton' or 'damped'")
        lo, hi = -np.inf if t_lo is None else t_lo, np.inf if t_hi is None else t_hi
        extra = []
        if solver == "damped":
            rule = _native.MLAT_RULE(_native.MLAT_SOLVER_LM, (_native.MLAT_RESTART if restart else 0) | (_native.MLAT_ALTITUDE if altitude else 0),
                                     int(min_rx), 0, float(alt_weight))
            fixes, aux, ms, mt = self.ctx.stream_mlat_rule(rule, lo, hi)
            extra = [("alt_ft", "<i4", aux["alt_ft"]), ("up_m", "<f8", aux["up_m"]), ("tries", "<i4", aux["tries"]), ("aux_flags", "<u4", aux["flags"])]
        else:
            fixes, ms, mt = self.ctx.stream_mlat(lo, hi, min_rx)
        out = np.zeros(len(fixes), dtype=np.dtype(_native.MLAT_DTYPE.descr + [("latitude", "<f8"), ("longitude", "<f8"), ("altitude_m", "<f8")] +
                                                  [(name, kind) for name, kind, _ in extra]))
        for name in _native.MLAT_DTYPE.names:
            out[name] = fixes[name]
        for j, f in enumerate(fixes):
            out["latitude"][j], out["longitude"][j], out["altitude_m"][j] = _native.ecef_to_geodetic(f["x"], f["y"], f["z"])
        for name, _, col in extra:
            out[name] = col
        return out, ms, mt

    def table(self, timestamp, ids=None, cutoff=None, mlat=False):
        """The lines the reference's print_planes draws ("Brief") for the merged picture at PDU timestamp `timestamp`.
        mlat=True: an aircraft without a position of its own (latitude NaN) that has a track is drawn at the track's latitude
        and longitude."""
        if not mlat:
            return _native.plane_table(self.merged(ids, cutoff)[0], timestamp)
        rows, _, track_of, tracks = self.merged(ids, cutoff, mlat=True)
        rows = rows.copy()
        fill = (track_of >= 0) & np.isnan(rows["latitude"])
        rows["latitude"][fill], rows["longitude"][fill] = tracks["latitude"][track_of[fill]], tracks["longitude"][track_of[fill]]
        return _native.plane_table(rows, timestamp)

    def state(self, i):
        """(pos, eob, n_overlong) of stream i"""
        return self.ctx.stream_state(i)

    @property
    def overlong(self):
        return sum(self.ctx.stream_state(i)[2] for i in range(self.n))

    def close(self):
        self.ctx.close_streams()


class MultiDevice:
    """ONE process, N devices, ONE host ring (BASELINE config 4 / SURVEY.md §8e as the reference's own process model:
    examples/adsb_rx.py:242-268 is one process with one IQ source).  Holds one context per device; process_host() hands a
    host buffer to adsb_process_sharded_multi: the stream is tiled into len(devices) * shards_per_device overlapped time
    shards, each device's feeder thread (inside the library, on the cpus local to its GPU) uploads and runs its shards
    ADSB_MAX_IN_FLIGHT deep, the seams are stitched on the host -- the result equals FrontEnd.process_format over the whole
    buffer bit for bit.  devices: HIP ordinals, e.g. range(torch.cuda.device_count()); an ordinal may repeat (several
    contexts on one GPU: how a one-GPU box exercises this)."""

    def __init__(self, fs, threshold, devices=(0,), flags=0, scales=None):
        self.fs, self.sps = float(fs), int(fs // 1e6)
        self.contexts = [_native.Context(fs, threshold, device=int(d), flags=int(flags)) for d in devices]
        for fmt, sc in (scales or {}).items():
            for cx in self.contexts:
                cx.set_format_scale(fmt, sc)
        self.last_stats = None

    def set_threshold(self, thr):
        for cx in self.contexts:
            cx.set_threshold(thr)

    def pinned(self, n_items, dtype):
        """Page-locked host ring near the FIRST device (one ring feeds every device; on a two-socket node the far socket's
        GPUs read it over the interconnect -- a caller with one ring per socket makes two MultiDevice objects)."""
        return _native.PinnedArray(n_items, dtype, near=self.contexts[0])

    def process_host(self, fmt, data, shards_per_device=1, abs_offset=0, out=None):
        recs, self.last_stats = _native.process_sharded_multi(self.contexts, fmt, data, shards_per_device, abs_offset, out=out,
                                                              want_stats=True)
        return recs

    def close(self):
        for cx in self.contexts:
            cx.close()
        self.contexts = []
