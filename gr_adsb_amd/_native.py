"""ctypes binding of libadsb_hip.so (C ABI: include/adsb_hip.h).

The product path: there is NO CPU implementation behind this module.  If the shared library is
missing, or no HIP device can be opened, the import / constructor raises -- it never falls back.
"""
import ctypes
import errno
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libadsb_hip.so")

BURST_DTYPE = np.dtype([("offset", "<i8"), ("peak", "<f4"), ("median", "<f4"), ("bits", "u1", (14,)), ("flags", "<u2")])
assert BURST_DTYPE.itemsize == 32

FLAG_TIMING = 1
FLAG_LONG_AWARE_GATE = 2  # opt-in: the gate holds 119*sps after a burst whose first data bit is set
FLAG_CONFIDENCE = 4       # opt-in: keep demod.bit_confidence's ratios (demod.py:97-101) for the whole-buffer entry points
FLAG_SINGLE_STREAM = 8    # profiling aid: the sparse tail of a pass on the compute stream instead of beside the next pass
FLAG_FRAMER_SLICES = 32   # adsb_framer_work also returns the 112 bits of tags whose burst ends inside the call's input
FLAG_NO_NUMA_BINDING = 64 # host side not placed on the GPU's NUMA node (default: page-locked buffers and copy threads are)
FLAG_LOW_LATENCY = 16     # the tail of a pass runs beside the next pass's k_detect: results a pass earlier, 1-2 % less throughput
FLAG_FEC_CONSERVATIVE = 128  # opt-in: the decoder's "Conservative" 1-2-bit burst repair on the device (decoder.py:738-780)
FLAG_AIRCRAFT_TABLE = 256    # opt-in: the decoder's aircraft table on the device: verdicts for address/parity replies
FLAG_DECODE = 512            # opt-in (with FLAG_AIRCRAFT_TABLE): the decoder's message decoding and plane fields on the device
FLAG_STREAM_DECODE = 1024    # opt-in: one decoder behind every receiver stream (open_streams), one device step per stream-batch call
FLAG_STREAM_DECODE_SHARED = 4096   # opt-in, with FLAG_STREAM_DECODE: ONE decoder behind all streams, fed every call's records in time order
FLAG_STREAM_DEDUP = 8192     # opt-in, with FLAG_STREAM_DECODE | FLAG_STREAM_DECODE_SHARED: a reply heard by several receivers is published once
FLAG_FEC_SOFT = 16384        # opt-in: soft-decision CRC repair of weak-bit errors from the samples behind the bits (include/adsb_hip.h SOFT REPAIR)
FLAG_FEC_SOFT_BATCH = 32768  # opt-in: the same repair in process_batch* / process_stream_batch*, each record against its own item's samples (SOFT REPAIR, IN A BATCH)
FLAG_PLANE_AGES = 2048       # opt-in, with FLAG_DECODE or FLAG_STREAM_DECODE: plane_dict's last_seen on the device (planes(seen=True), expire_*)
# include/adsb_hip.h adsb_decoded: one row per delivered record of a FLAG_DECODE context
DECODED_DTYPE = np.dtype([("port", "u1"), ("df", "u1"), ("present", "u1"), ("pad0", "u1"), ("icao", "<i4"), ("bits", "u1", (14,)),
                          ("callsign", "S8"), ("pad1", "u1", (2,)), ("altitude", "<i4"), ("velocity_we", "<i4"),
                          ("velocity_sn", "<i4"), ("vertical_rate", "<i4"), ("latitude", "<f8"), ("longitude", "<f8"),
                          ("num_msgs", "<u4"), ("pad2", "<u4")])
assert DECODED_DTYPE.itemsize == 72
DEC_NONE, DEC_DECODED, DEC_UNKNOWN, DEC_RAISED = 0, 1, 2, 3
DEC_DUPLICATE = 4            # FLAG_STREAM_DEDUP: another receiver's hearing of this reply was published, this one was not
DEC_HAS_PLANE, DEC_HAS_CALLSIGN, DEC_HAS_ALTITUDE, DEC_HAS_VELOCITY = 1, 2, 4, 8
DEC_MSG_FILTERS = {"All Messages": 0, "Extended Squitter Only": 1}
ABI_VERSION = 5
# include/adsb_hip.h adsb_soft_fix: one row per delivered record (per tag: demod_work) of a FLAG_FEC_SOFT context
SOFT_DTYPE = np.dtype([("nflip", "u1"), ("ncand", "u1"), ("bit", "u1", (5,)), ("pad", "u1")])
assert SOFT_DTYPE.itemsize == 8
SOFT_FEC_DEFAULTS = dict(n_weak=8, max_flips=3, min_key=0.0)


class SOFT_FEC_RULE(ctypes.Structure):
    _fields_ = [("n_weak", ctypes.c_int32), ("max_flips", ctypes.c_int32), ("min_key", ctypes.c_float), ("flags", ctypes.c_uint32)]


# input sample formats (include/adsb_hip.h ADSB_FMT_*): numpy dtype of the flat host array, items per sample
FMT_FC32, FMT_MAG2, FMT_SC16, FMT_SC8, FMT_CU8 = 0, 1, 2, 3, 4
FMT_LAYOUT = {FMT_FC32: (np.complex64, 1), FMT_MAG2: (np.float32, 1), FMT_SC16: (np.int16, 2), FMT_SC8: (np.int8, 2),
              FMT_CU8: (np.uint8, 2)}
FMT_BYTES = {FMT_FC32: 8, FMT_MAG2: 4, FMT_SC16: 4, FMT_SC8: 2, FMT_CU8: 2}
BURST_DEMOD = 1
BURST_KEPT = 2
BURST_PARITY_OK = 32     # Mode S parity pre-filter bits (include/adsb_hip.h; decoder.py:550-688)
BURST_LONG = 64
BURST_KNOWN_DF = 128
BURST_DF_SHIFT = 8
BURST_LONG_HINT = 0x2000 # records of a long-aware context: this burst holds the gate for 119*sps
BURST_FEC_FIXED = 0x4000 # FLAG_FEC_CONSERVATIVE: bits repaired, the pre-filter bits are the repaired reply's
BURST_FEC_DF = 0x8000    # FLAG_FEC_CONSERVATIVE: the decoder's repair would change the DF; bits left raw
BURST_AP_FEC = 0x0004    # FLAG_AIRCRAFT_TABLE + FLAG_FEC_CONSERVATIVE: AA unknown, the decoder's repair accepts the reply
BURST_AP_KNOWN = 0x0008  # FLAG_AIRCRAFT_TABLE: the AA of this address/parity reply was announced by an earlier PDU
MAX_IN_FLIGHT = 3
# one item of adsb_process_batch* (include/adsb_hip.h: adsb_batch_item): pointer, samples, stream offset, threshold
BATCH_ITEM_DTYPE = np.dtype([("data", "<u8"), ("n", "<i8"), ("abs_offset", "<i8"), ("threshold", "<f4"), ("reserved", "<u4")])
assert BATCH_ITEM_DTYPE.itemsize == 32
BATCH_ITEM_MAX = 1 << 22     # ADSB_BATCH_ITEM_MAX: longer items take the ordinary pass inside the call
# one item of adsb_process_stream_batch* (adsb_stream_item): pointer, samples, stream id, flags (STREAM_END), threshold
STREAM_ITEM_DTYPE = np.dtype([("data", "<u8"), ("n", "<i8"), ("stream", "<i4"), ("flags", "<u4"), ("threshold", "<f4"),
                              ("reserved", "<u4")])
assert STREAM_ITEM_DTYPE.itemsize == 32
# one entry of adsb_stream_planes_merged's info (adsb_merged): info[j] belongs to rows[j]
MERGED_DTYPE = np.dtype([("last_seen", "<i8"), ("n_streams", "<i4"), ("src_callsign", "<i4"), ("src_altitude", "<i4"),
                         ("src_velocity", "<i4"), ("src_position", "<i4"), ("pad", "<i4")])
assert MERGED_DTYPE.itemsize == 32
# one row of adsb_stream_mlat (adsb_mlat_fix): the members of row j are member_stream / member_ts[first .. first + n_rx)
MLAT_DTYPE = np.dtype([("ts", "<f8"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("t_tx", "<f8"), ("rms_m", "<f8"), ("bits", "u1", (14,)),
                       ("flags", "<u2"), ("icao", "<i4"), ("n_rx", "<i4"), ("n_heard", "<i4"), ("status", "<i4"), ("iters", "<i4"),
                       ("first", "<i4")])
assert MLAT_DTYPE.itemsize == 88
MLAT_OK, MLAT_NO_CONVERGE, MLAT_SINGULAR = 0, 1, 2       # ADSB_MLAT_*
MLAT_C = 299702547.0         # ADSB_MLAT_C, m/s
# adsb_stream_mlat_rule: the rule a caller states (adsb_mlat_rule) and the row beside each fix (adsb_mlat_aux)
MLAT_SOLVER_GN, MLAT_SOLVER_LM = 0, 1                     # ADSB_MLAT_SOLVER_*
MLAT_RESTART, MLAT_ALTITUDE = 1, 2                       # ADSB_MLAT_RESTART, ADSB_MLAT_ALTITUDE
MLAT_AUX_AIDED, MLAT_AUX_RESTARTED, MLAT_AUX_SECOND_KEPT = 1, 2, 4
MLAT_AUX_DTYPE = np.dtype([("up_m", "<f8"), ("lambda", "<f8"), ("alt_ft", "<i4"), ("tries", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
assert MLAT_AUX_DTYPE.itemsize == 32


class MLAT_RULE(ctypes.Structure):
    _fields_ = [("solver", ctypes.c_int32), ("flags", ctypes.c_int32), ("min_rx", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("alt_weight", ctypes.c_double)]


assert ctypes.sizeof(MLAT_RULE) == 24
# the MLAT track store (include/adsb_hip.h MLAT TRACKS): one row of adsb_stream_mlat_tracks (adsb_mlat_track), the filter rule
# a caller states (adsb_mlat_track_rule) and one update's totals (adsb_mlat_track_stats)
TRACK_GAP, TRACK_RESTARTED = 1, 2                         # ADSB_TRACK_*
MLAT_TRACK_DTYPE = np.dtype([("icao", "<i4"), ("flags", "<u4"), ("n_fixes", "<i4"), ("n_rejected", "<i4"), ("first_ts", "<f8"), ("last_ts", "<f8"),
                             ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("vz", "<f8"), ("rms_m", "<f8"),
                             ("n_rx", "<i4"), ("misses", "<i4")])
assert MLAT_TRACK_DTYPE.itemsize == 96


class MLAT_TRACK_RULE(ctypes.Structure):
    _fields_ = [("alpha", ctypes.c_double), ("beta", ctypes.c_double), ("gate_m", ctypes.c_double), ("max_speed_mps", ctypes.c_double),
                ("max_gap_s", ctypes.c_double), ("max_rms_m", ctypes.c_double), ("min_up_m", ctypes.c_double),
                ("restart_after", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MLAT_TRACK_STATS(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int64) for name in ("fixes", "eligible", "unusable", "stale", "rejected", "taken", "started", "tracks")]


assert ctypes.sizeof(MLAT_TRACK_RULE) == 64 and ctypes.sizeof(MLAT_TRACK_STATS) == 64
# the Python layer's defaults of the track rule (the C call has none)
MLAT_TRACK_DEFAULTS = dict(alpha=0.3, beta=0.05, gate_m=2000.0, max_speed_mps=350.0, max_gap_s=30.0, max_rms_m=500.0, min_up_m=0.0, restart_after=3)


def mlat_track_rule(**kw):
    """-> MLAT_TRACK_RULE: MLAT_TRACK_DEFAULTS with the keywords given over them"""
    unknown = set(kw) - set(MLAT_TRACK_DEFAULTS)
    if unknown:
        raise TypeError("unknown track rule field(s): %s" % ", ".join(sorted(unknown)))
    v = dict(MLAT_TRACK_DEFAULTS)
    v.update(kw)
    return MLAT_TRACK_RULE(float(v["alpha"]), float(v["beta"]), float(v["gate_m"]), float(v["max_speed_mps"]), float(v["max_gap_s"]),
                           float(v["max_rms_m"]), float(v["min_up_m"]), int(v["restart_after"]), 0)


INT64_MIN = -(1 << 63)       # the cutoff that hides nothing
STREAM_END = 1               # ADSB_STREAM_END: the stream's last item
STREAM_FRESH_EOB = -(1 << 61)    # the carried end-of-burst offset of a fresh stream

EXPORTS = [
    "adsb_abi_version", "adsb_create", "adsb_destroy", "adsb_set_threshold", "adsb_set_stream", "adsb_set_copy_threads", "adsb_host_copy", "adsb_wait_for_event", "adsb_reset", "adsb_framer_state",
    "adsb_process_iq", "adsb_process_mag2", "adsb_process_iq_device", "adsb_process_mag2_device", "adsb_last_result",
    "adsb_submit_iq_device", "adsb_submit_mag2_device", "adsb_submit_iq16_device", "adsb_submit_shard_device", "adsb_wait",
    "adsb_set_iq16_scale", "adsb_process_iq16", "adsb_process_iq16_device",
    "adsb_set_format_scale", "adsb_process_format", "adsb_process_format_device", "adsb_submit_format_device",
    "adsb_submit_format_host", "adsb_last_confidence", "adsb_set_soft_fec", "adsb_last_soft", "adsb_batch_last_soft", "adsb_mode_s_soft_fec", "adsb_set_decoder", "adsb_last_decoded", "adsb_decode_pdus",
    "adsb_framer_work", "adsb_framer_work_passthrough", "adsb_demod_work", "adsb_shard_bounds", "adsb_process_sharded_device", "adsb_shard_device", "adsb_shard_host", "adsb_shard_fixup", "adsb_stitch", "adsb_snr_db", "adsb_mode_s_syndrome", "adsb_mode_s_fec", "adsb_mode_s_aircraft", "adsb_plan_chunks", "adsb_get_stats",
    "adsb_process_sharded_multi", "adsb_device_alloc", "adsb_device_free", "adsb_device_upload", "adsb_clear_pending_events",
    "adsb_process_batch_device", "adsb_process_batch",
    "adsb_streams_open", "adsb_streams_close", "adsb_stream_set_base", "adsb_stream_state", "adsb_stream_reset",
    "adsb_process_stream_batch", "adsb_process_stream_batch_device",
    "adsb_streams_set_decoder", "adsb_stream_set_start", "adsb_stream_last_decoded", "adsb_stream_decoder_reserve",
    "adsb_stream_decoder_stats", "adsb_planes", "adsb_stream_planes",
    "adsb_planes_seen", "adsb_stream_planes_seen", "adsb_planes_expire", "adsb_stream_planes_expire",
    "adsb_stream_planes_merged", "adsb_stream_last_order", "adsb_streams_decoder_reset",
    "adsb_streams_set_dedup", "adsb_stream_last_duplicates", "adsb_stream_dedup_stats",
    "adsb_stream_set_ecef", "adsb_stream_mlat", "adsb_stream_mlat_rule", "adsb_stream_mlat_stats", "adsb_geodetic_to_ecef", "adsb_ecef_to_geodetic",
    "adsb_stream_mlat_track", "adsb_stream_mlat_tracks", "adsb_stream_mlat_tracks_expire", "adsb_stream_mlat_tracks_reset",
    "adsb_reset_stats", "adsb_detect_history", "adsb_numa_info", "adsb_host_alloc_near", "adsb_last_error", "adsb_host_alloc", "adsb_host_free", "adsb_host_register", "adsb_host_unregister",
]


class Stats(ctypes.Structure):
    _fields_ = [("detect_launches", ctypes.c_uint64), ("detect_ms", ctypes.c_double), ("detect_samples", ctypes.c_uint64),
                ("detect_bytes", ctypes.c_uint64), ("calls", ctypes.c_uint64), ("retries", ctypes.c_uint64),
                ("longrun_calls", ctypes.c_uint64), ("detect_grid", ctypes.c_uint64), ("blocks_per_cu", ctypes.c_uint64),
                ("detect_gap_ms", ctypes.c_double), ("detect_gaps", ctypes.c_uint64), ("longrun_pulses", ctypes.c_uint64),
                ("poll_fallbacks", ctypes.c_uint64), ("shard_fallbacks", ctypes.c_uint64)]


MULTI_MAX_CTX = 64


class MultiStats(ctypes.Structure):
    _fields_ = [("contexts", ctypes.c_int32), ("shards", ctypes.c_int32), ("fallbacks", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("wall_s", ctypes.c_double), ("feeder_s", ctypes.c_double * MULTI_MAX_CTX),
                ("device", ctypes.c_int32 * MULTI_MAX_CTX), ("numa_node", ctypes.c_int32 * MULTI_MAX_CTX)]


class AdsbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libadsb_hip: error %d (%s)%s" % (code, os.strerror(-code) if code < 0 else "?", ": " + msg if msg else ""))
        self.code = code


_lib = None


def geodetic_to_ecef(lat_deg, lon_deg, alt_m):
    """WGS-84 degrees and metres -> ECEF (x, y, z) in metres (adsb_geodetic_to_ecef: plain host arithmetic)."""
    x, y, z = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    load().adsb_geodetic_to_ecef(float(lat_deg), float(lon_deg), float(alt_m), ctypes.byref(x), ctypes.byref(y), ctypes.byref(z))
    return x.value, y.value, z.value


def ecef_to_geodetic(x, y, z):
    """ECEF metres -> WGS-84 (latitude, longitude, altitude) in degrees and metres (adsb_ecef_to_geodetic)."""
    la, lo, al = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    load().adsb_ecef_to_geodetic(float(x), float(y), float(z), ctypes.byref(la), ctypes.byref(lo), ctypes.byref(al))
    return la.value, lo.value, al.value


def load():
    """dlopen the in-tree library; raises if it has not been built (python -m gr_adsb_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (same soname): import it FIRST so that this library binds to the
    # runtime torch uses; loading ours first and torch afterwards puts two runtimes in one process and
    # device discovery then fails in the second one.
    import sys
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    path = os.environ.get("ADSB_HIP_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise ImportError("libadsb_hip.so not built: run `python -m gr_adsb_amd.build` (hipcc, gfx950). "
                          "There is no CPU fallback for the ADS-B hot path.")
    lib = ctypes.CDLL(path)
    c = ctypes
    vp, i64, i32, f32 = c.c_void_p, c.c_int64, c.c_int32, c.c_float
    lib.adsb_abi_version.restype = c.c_int
    lib.adsb_create.argtypes = [c.c_double, f32, c.c_int, c.c_uint32, c.POINTER(vp)]
    lib.adsb_destroy.argtypes = [vp]
    lib.adsb_destroy.restype = None
    lib.adsb_set_threshold.argtypes = [vp, f32]
    lib.adsb_set_stream.argtypes = [vp, vp]
    lib.adsb_reset.argtypes = [vp]
    lib.adsb_wait_for_event.argtypes = [vp, vp]
    lib.adsb_set_copy_threads.argtypes = [vp, i32]
    lib.adsb_host_copy.argtypes = [vp, vp, vp, c.c_size_t]
    lib.adsb_framer_state.argtypes = [vp, c.POINTER(c.c_float), c.POINTER(c.c_int64)]
    lib.adsb_set_iq16_scale.argtypes = [vp, f32]
    lib.adsb_submit_iq16_device.argtypes = [vp, vp, i64, i64, c.POINTER(i32)]
    for name in ("adsb_process_iq", "adsb_process_mag2", "adsb_process_iq_device", "adsb_process_mag2_device",
                 "adsb_process_iq16", "adsb_process_iq16_device"):
        getattr(lib, name).argtypes = [vp, vp, i64, i64, vp, i32, c.POINTER(i32)]
    lib.adsb_set_format_scale.argtypes = [vp, c.c_int, f32]
    lib.adsb_process_format.argtypes = [vp, c.c_int, vp, i64, i64, vp, i32, c.POINTER(i32)]
    lib.adsb_process_format_device.argtypes = [vp, c.c_int, vp, i64, i64, vp, i32, c.POINTER(i32)]
    lib.adsb_submit_format_device.argtypes = [vp, c.c_int, vp, i64, i64, c.POINTER(i32)]
    lib.adsb_submit_format_host.argtypes = [vp, c.c_int, vp, i64, i64, c.POINTER(i32)]
    lib.adsb_last_confidence.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_set_decoder.argtypes = [vp, i32, c.c_double]
    lib.adsb_last_decoded.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_decode_pdus.argtypes = [vp, vp, vp, i32, vp]
    lib.adsb_last_result.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_submit_iq_device.argtypes = [vp, vp, i64, i64, c.POINTER(i32)]
    lib.adsb_submit_mag2_device.argtypes = [vp, vp, i64, i64, c.POINTER(i32)]
    lib.adsb_wait.argtypes = [vp, i32, vp, i32, c.POINTER(i32)]
    lib.adsb_submit_shard_device.argtypes = [vp, c.c_int, vp, i64, i64, i64, i64, i64, i32, c.POINTER(i32)]
    lib.adsb_framer_work.argtypes = [vp, vp, i64, i64, i64, vp, i32, c.POINTER(i32)]
    lib.adsb_framer_work_passthrough.argtypes = [vp, vp, i64, i64, i64, vp, vp, i32, c.POINTER(i32)]
    lib.adsb_demod_work.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, vp]
    lib.adsb_shard_device.argtypes = [vp, c.c_int, vp, i64, i64, i64, i64, i64, i32, vp, i32, c.POINTER(i32)]
    lib.adsb_shard_host.argtypes = [vp, c.c_int, vp, i64, i64, i64, i64, i64, i32, c.c_uint32, vp, i32, c.POINTER(i32)]
    lib.adsb_shard_fixup.argtypes = [vp, i32, c.c_int, i64, c.POINTER(i32)]
    lib.adsb_shard_bounds.argtypes = [i64, i32, i32, c.c_int, i64, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.adsb_shard_bounds.restype = c.c_int32
    lib.adsb_process_sharded_device.argtypes = [vp, c.c_int, vp, i64, i64, i32, vp, i32, c.POINTER(i32)]
    lib.adsb_process_sharded_multi.argtypes = [c.POINTER(vp), i32, c.c_int, vp, i64, i64, i32, vp, i32, c.POINTER(i32), c.POINTER(MultiStats)]
    for name in ("adsb_process_batch_device", "adsb_process_batch", "adsb_process_stream_batch_device", "adsb_process_stream_batch"):
        getattr(lib, name).argtypes = [vp, c.c_int, vp, i32, vp, i32, vp, c.POINTER(i32), c.POINTER(i32)]
    lib.adsb_streams_open.argtypes = [vp, i32]
    lib.adsb_streams_close.argtypes = [vp]
    lib.adsb_stream_set_base.argtypes = [vp, i32, i64]
    lib.adsb_stream_state.argtypes = [vp, i32, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.adsb_stream_reset.argtypes = [vp, i32]
    lib.adsb_streams_set_decoder.argtypes = [vp, i32]
    lib.adsb_stream_set_start.argtypes = [vp, i32, c.c_double]
    lib.adsb_stream_last_decoded.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_stream_last_order.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_streams_decoder_reset.argtypes = [vp]
    lib.adsb_streams_set_dedup.argtypes = [vp, c.c_double, c.c_double]
    lib.adsb_stream_last_duplicates.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_stream_dedup_stats.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(c.c_double)]
    lib.adsb_stream_set_ecef.argtypes = [vp, i32, c.c_double, c.c_double, c.c_double]
    lib.adsb_stream_mlat.argtypes = [vp, c.c_double, c.c_double, i32, vp, i32, c.POINTER(i32), vp, vp, i32, c.POINTER(i32)]
    lib.adsb_stream_mlat_rule.argtypes = [vp, c.c_double, c.c_double, c.POINTER(MLAT_RULE), vp, vp, i32, c.POINTER(i32), vp, vp, i32, c.POINTER(i32)]
    lib.adsb_stream_mlat_stats.argtypes = [vp, c.POINTER(i32), c.POINTER(c.c_double)]
    lib.adsb_stream_mlat_track.argtypes = [vp, c.c_double, c.c_double, c.POINTER(MLAT_RULE), c.POINTER(MLAT_TRACK_RULE), c.POINTER(MLAT_TRACK_STATS)]
    lib.adsb_stream_mlat_tracks.argtypes = [vp, i32, c.c_double, vp, i32, c.POINTER(i32)]
    lib.adsb_stream_mlat_tracks_expire.argtypes = [vp, c.c_double, c.POINTER(c.c_int64)]
    lib.adsb_stream_mlat_tracks_reset.argtypes = [vp]
    lib.adsb_geodetic_to_ecef.argtypes = [c.c_double] * 3 + [c.POINTER(c.c_double)] * 3
    lib.adsb_geodetic_to_ecef.restype = None
    lib.adsb_ecef_to_geodetic.argtypes = [c.c_double] * 3 + [c.POINTER(c.c_double)] * 3
    lib.adsb_ecef_to_geodetic.restype = None
    lib.adsb_stream_decoder_reserve.argtypes = [vp, i64]
    lib.adsb_stream_decoder_stats.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.adsb_planes.argtypes = [vp, vp, i32, c.POINTER(i32)]
    lib.adsb_stream_planes.argtypes = [vp, vp, i32, vp, i32, vp, c.POINTER(i32)]
    lib.adsb_planes_seen.argtypes = [vp, vp, vp, i32, c.POINTER(i32)]
    lib.adsb_stream_planes_seen.argtypes = [vp, vp, i32, vp, vp, i32, vp, c.POINTER(i32)]
    lib.adsb_planes_expire.argtypes = [vp, c.c_int64, c.POINTER(c.c_int64)]
    lib.adsb_stream_planes_expire.argtypes = [vp, vp, i32, vp, c.POINTER(c.c_int64)]
    lib.adsb_stream_planes_merged.argtypes = [vp, vp, i32, c.c_int64, vp, vp, i32, c.POINTER(i32)]
    lib.adsb_device_alloc.argtypes = [vp, c.POINTER(vp), c.c_size_t]
    lib.adsb_device_free.argtypes = [vp, vp]
    lib.adsb_device_upload.argtypes = [vp, vp, vp, c.c_size_t]
    lib.adsb_clear_pending_events.argtypes = [vp]
    lib.adsb_stitch.argtypes = [vp, i32, c.c_int, c.POINTER(i32)]
    lib.adsb_snr_db.argtypes = [f32, f32]
    lib.adsb_snr_db.restype = f32
    lib.adsb_mode_s_syndrome.argtypes = [vp, c.POINTER(i32), c.POINTER(i32)]
    lib.adsb_mode_s_syndrome.restype = c.c_uint32
    lib.adsb_mode_s_fec.argtypes = [vp, vp, c.POINTER(i32), c.POINTER(i32)]
    lib.adsb_mode_s_fec.restype = c.c_uint32
    lib.adsb_mode_s_soft_fec.argtypes = [vp, vp, c.POINTER(SOFT_FEC_RULE), vp, vp]
    lib.adsb_mode_s_soft_fec.restype = c.c_uint32
    lib.adsb_set_soft_fec.argtypes = [vp, c.POINTER(SOFT_FEC_RULE)]
    lib.adsb_last_soft.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_batch_last_soft.argtypes = [vp, c.POINTER(vp), c.POINTER(i32)]
    lib.adsb_mode_s_aircraft.argtypes = [vp, i32, c.POINTER(i32), c.POINTER(i32), c.POINTER(i32)]
    lib.adsb_mode_s_aircraft.restype = c.c_uint32
    lib.adsb_plan_chunks.argtypes = [i64, i64, c.POINTER(i64), c.POINTER(i64)]
    lib.adsb_plan_chunks.restype = c.c_int32
    lib.adsb_get_stats.argtypes = [vp, c.POINTER(Stats)]
    lib.adsb_reset_stats.argtypes = [vp]
    lib.adsb_detect_history.argtypes = [vp, vp, i32, c.POINTER(i32)]
    lib.adsb_numa_info.argtypes = [vp, c.POINTER(i32), c.c_char_p, c.c_size_t, c.c_char_p, c.c_size_t]
    lib.adsb_host_alloc_near.argtypes = [vp, c.POINTER(vp), c.c_size_t]
    lib.adsb_host_alloc.argtypes = [c.POINTER(vp), c.c_size_t]
    lib.adsb_host_free.argtypes = [vp]
    lib.adsb_host_register.argtypes = [vp, c.c_size_t]
    lib.adsb_host_unregister.argtypes = [vp]
    lib.adsb_last_error.argtypes = [vp]
    lib.adsb_last_error.restype = c.c_char_p
    _lib = lib
    return lib


class Context:
    """Owns one adsb_ctx (one HIP device + stream).  Thin: every method is one C-ABI call."""

    def __init__(self, fs, threshold, device=0, flags=0):
        self.lib = load()
        self.fs = float(fs)
        self.sps = int(fs // 1e6)
        self._h = ctypes.c_void_p()
        self._thr = np.float32(threshold)
        self.last_batch_fallbacks = 0
        self.flags = int(flags)
        rc = self.lib.adsb_create(float(fs), float(np.float32(threshold)), int(device), int(flags), ctypes.byref(self._h))
        if rc != 0:
            self._h = ctypes.c_void_p()
            raise AdsbError(rc, "adsb_create(fs=%r, device=%r) failed; a HIP device is required" % (fs, device))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.adsb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise AdsbError(rc, self.lib.adsb_last_error(self._h).decode("utf-8", "replace"))

    def set_threshold_cached(self, thr):
        """set_threshold, skipped while the value is unchanged (the blocks call this once per work())."""
        if thr != getattr(self, "_thr_cached", None):
            self.set_threshold(thr)

    def set_threshold(self, thr):
        self._chk(self.lib.adsb_set_threshold(self._h, float(np.float32(thr))))
        self._thr_cached = thr
        self._thr = np.float32(thr)

    def set_stream(self, stream_handle):
        self._chk(self.lib.adsb_set_stream(self._h, ctypes.c_void_p(int(stream_handle))))

    def reset(self):
        self._chk(self.lib.adsb_reset(self._h))

    # The three calls every input format has (FMT_LAYOUT: dtype and items per sample of the flat host array); the methods
    # named after one format below are these with that format.
    def _host(self, fmt, data, abs_offset):
        dt, per = FMT_LAYOUT[fmt]
        data = np.ascontiguousarray(data, dtype=dt)
        n_out = ctypes.c_int32(0)
        self._chk(self.lib.adsb_process_format(self._h, fmt, ctypes.c_void_p(data.ctypes.data), len(data) // per,
                                               int(abs_offset), None, 0, ctypes.byref(n_out)))
        return self.last_result()

    def _device(self, fmt, dev_ptr, n, abs_offset, fetch):
        n_out = ctypes.c_int32(0)
        self._chk(self.lib.adsb_process_format_device(self._h, fmt, ctypes.c_void_p(int(dev_ptr)), int(n), int(abs_offset),
                                                      None, 0, ctypes.byref(n_out)))
        return self.last_result() if fetch else n_out.value

    def _submit(self, fmt, dev_ptr, n, abs_offset):
        t = ctypes.c_int32(-1)
        self._chk(self.lib.adsb_submit_format_device(self._h, fmt, ctypes.c_void_p(int(dev_ptr)), int(n), int(abs_offset),
                                                     ctypes.byref(t)))
        return t.value

    def last_result(self, copy=True):
        """Bursts of the last finished call.  copy=False returns a writable view of the context's pinned
        buffer, valid until the same pipeline slot is used again (MAX_IN_FLIGHT submissions later)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_last_result(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=BURST_DTYPE)
        buf = (ctypes.c_char * (n.value * 32)).from_address(p.value)
        v = np.frombuffer(buf, dtype=BURST_DTYPE)
        return v.copy() if copy else v

    def last_confidence(self, copy=True):
        """FLAG_CONFIDENCE contexts: float32 [n,112] ratios bit1_amp / bit0_amp of the last finished call's bursts
        (demod.py:91-101); confidence_db() turns them into demod.bit_confidence."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_last_confidence(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros((0, 112), dtype=np.float32)
        buf = (ctypes.c_char * (n.value * 112 * 4)).from_address(p.value)
        v = np.frombuffer(buf, dtype=np.float32).reshape(n.value, 112)
        return v.copy() if copy else v

    def set_soft_fec(self, n_weak=8, max_flips=3, min_key=0.0):
        """FLAG_FEC_SOFT and FLAG_FEC_SOFT_BATCH contexts: the soft repair's rule (adsb_set_soft_fec): the n_weak weakest bits are candidates, at most
        max_flips of them are flipped, a candidate's weakness is at least min_key."""
        rule = SOFT_FEC_RULE(int(n_weak), int(max_flips), float(min_key), 0)
        self._chk(self.lib.adsb_set_soft_fec(self._h, ctypes.byref(rule)))

    def last_soft(self, copy=True):
        """FLAG_FEC_SOFT contexts: SOFT_DTYPE rows of the last finished call's records, or of the last demod_work's tags
        (adsb_last_soft): nflip != 0 marks a record the soft rule repaired, bit[] names the flipped bits."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_last_soft(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=SOFT_DTYPE)
        buf = (ctypes.c_char * (n.value * SOFT_DTYPE.itemsize)).from_address(p.value)
        v = np.frombuffer(buf, dtype=SOFT_DTYPE)
        return v.copy() if copy else v

    def last_batch_soft(self):
        """FLAG_FEC_SOFT_BATCH contexts: SOFT_DTYPE rows of the last process_batch* / process_stream_batch* call, row t for its
        record t (adsb_batch_last_soft); a copy."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_batch_last_soft(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=SOFT_DTYPE)
        buf = (ctypes.c_char * (n.value * SOFT_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=SOFT_DTYPE).copy()

    def set_decoder(self, msg_filter="All Messages", start_timestamp=0.0):
        """FLAG_DECODE contexts: the decoder's msg_filter and the start timestamp of the records' PDUs (adsb_set_decoder)."""
        self._chk(self.lib.adsb_set_decoder(self._h, DEC_MSG_FILTERS[msg_filter], float(start_timestamp)))

    def last_decoded(self, copy=True):
        """FLAG_DECODE contexts: DECODED_DTYPE rows of the last finished call's records (adsb_last_decoded)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_last_decoded(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=DECODED_DTYPE)
        buf = (ctypes.c_char * (n.value * DECODED_DTYPE.itemsize)).from_address(p.value)
        v = np.frombuffer(buf, dtype=DECODED_DTYPE)
        return v.copy() if copy else v

    def decode_pdus(self, bits14, timestamps):
        """FLAG_DECODE contexts: decode already-published PDUs (n x 14 packed bytes, n float64 timestamps) through the context's
        decoder state, in one device call (adsb_decode_pdus) -> DECODED_DTYPE rows."""
        b = np.ascontiguousarray(bits14, dtype=np.uint8).reshape(-1, 14)
        t = np.ascontiguousarray(timestamps, dtype=np.float64).reshape(-1)
        assert len(b) == len(t)
        rows = np.zeros(len(b), dtype=DECODED_DTYPE)
        self._chk(self.lib.adsb_decode_pdus(self._h, b.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p),
                                            len(b), rows.ctypes.data_as(ctypes.c_void_p)))
        return rows

    def _snapshot(self, call, cap, seen=False):
        """call(rows pointer, cap, n_out) -> rc; the buffer starts at cap rows and is sized by the count the call reports when
        that was too small (-ENOSPC), once.  seen: call(rows pointer, last_seen pointer, cap, n_out) -> (rows, last_seen)."""
        n = ctypes.c_int32(0)
        for _ in range(2):
            rows = np.zeros(max(int(cap), 0), dtype=DECODED_DTYPE)
            rp = ctypes.c_void_p(rows.ctypes.data) if len(rows) else None
            if seen:
                ages = np.zeros(len(rows), dtype=np.int64)
                rc = call(rp, ctypes.c_void_p(ages.ctypes.data) if len(rows) else None, len(rows), ctypes.byref(n))
            else:
                rc = call(rp, len(rows), ctypes.byref(n))
            if rc != -28:
                break
            cap = n.value
        self._chk(rc)
        return (rows[:n.value], ages[:n.value]) if seen else rows[:n.value]

    def planes(self, cap=None, seen=False):
        """FLAG_DECODE contexts: a snapshot of the decoder's plane table (adsb_planes) -> DECODED_DTYPE rows, one per aircraft in
        ascending address order (port DEC_NONE, df 0, bits zero; plane_entry turns one into the reference's plane_dict entry).
        cap: the first buffer's rows (None: a count query first).  seen (FLAG_PLANE_AGES contexts; adsb_planes_seen):
        (rows, last_seen), last_seen[j] the int64 clock of rows[j]'s last update_plane."""
        if seen:
            return self._snapshot(lambda r, a, k, n: self.lib.adsb_planes_seen(self._h, r, a, k, n), 0 if cap is None else cap, True)
        return self._snapshot(lambda r, k, n: self.lib.adsb_planes(self._h, r, k, n), 0 if cap is None else cap)

    def expire_planes(self, cutoff):
        """FLAG_DECODE | FLAG_PLANE_AGES contexts: remove every plane with last_seen < cutoff as `del plane_dict[key]` does
        (adsb_planes_expire) -> the number removed."""
        n = ctypes.c_int64(0)
        self._chk(self.lib.adsb_planes_expire(self._h, int(cutoff), ctypes.byref(n)))
        return n.value

    def expire_stream_planes(self, cutoffs, streams=None):
        """FLAG_STREAM_DECODE | FLAG_PLANE_AGES contexts: remove every plane of the i-th selected stream (streams: strictly
        ascending indices, None: all) with last_seen < cutoffs[i] (adsb_stream_planes_expire) -> the number removed."""
        cut = np.ascontiguousarray(cutoffs, dtype=np.int64).reshape(-1)
        if streams is None:
            sp, k = None, 0
            want = self._n_streams()
        else:
            sel = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
            check_stream_selection(sel, self._n_streams())
            want = k = len(sel)
            sp = ctypes.c_void_p(sel.ctypes.data) if k else ctypes.c_void_p(cut.ctypes.data)
        if len(cut) != want:
            raise ValueError("one cutoff per selected stream: %d for %d" % (len(cut), want))
        n = ctypes.c_int64(0)
        self._chk(self.lib.adsb_stream_planes_expire(self._h, sp, k, ctypes.c_void_p(cut.ctypes.data) if len(cut) else None,
                                                     ctypes.byref(n)))
        return n.value

    def stream_planes(self, streams=None, cap=None, seen=False):
        """FLAG_STREAM_DECODE contexts: a snapshot of the streams' plane tables (adsb_stream_planes) -> (rows, first): rows
        ordered by (stream, address), first[i]:first[i + 1] those of the i-th selected stream.  streams: strictly ascending
        stream indices, None: all of them.  cap: the first buffer's rows (None: stream_decoder_stats' plane count).
        seen (FLAG_PLANE_AGES contexts; adsb_stream_planes_seen): (rows, last_seen, first)."""
        if streams is None:
            sel, k = None, 0
            first = np.zeros(self._n_streams() + 1, dtype=np.int32)
        else:
            sel = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
            check_stream_selection(sel, self._n_streams())
            k = len(sel)
            first = np.zeros(k + 1, dtype=np.int32)
        sp = None if sel is None else ctypes.c_void_p(sel.ctypes.data) if k else ctypes.c_void_p(first.ctypes.data)
        fp = ctypes.c_void_p(first.ctypes.data)
        cap = self.stream_decoder_stats()[0] if cap is None else cap
        if seen:
            rows, ages = self._snapshot(lambda r, a, c_, n: self.lib.adsb_stream_planes_seen(self._h, sp, k, r, a, c_, fp, n), cap, True)
            return rows, ages, first
        rows = self._snapshot(lambda r, c_, n: self.lib.adsb_stream_planes(self._h, sp, k, r, c_, fp, n), cap)
        return rows, first

    def merged_planes(self, streams=None, cutoff=None, cap=None):
        """FLAG_STREAM_DECODE | FLAG_PLANE_AGES contexts: the selected streams' plane tables folded into one
        (adsb_stream_planes_merged) -> (rows, info): one DECODED_DTYPE row per aircraft in ascending address order and its
        MERGED_DTYPE entry.  Per field group (callsign, altitude, velocity, position) the row shows the entry with the
        greatest last_seen that has the group (ties: the lowest stream), info["src_*"] names that stream (-1: nobody has it);
        num_msgs is the sum, info["last_seen"] the largest.  streams: strictly ascending indices, None: all.  cutoff: entries
        with last_seen < cutoff are hidden (None: INT64_MIN, nothing is).  cap: the first buffer's rows (None: a count query
        first)."""
        if streams is None:
            sel, k, sp = None, 0, None
        else:
            sel = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
            check_stream_selection(sel, self._n_streams())
            k = len(sel)
        cut = INT64_MIN if cutoff is None else int(cutoff)
        n = ctypes.c_int32(0)
        if sel is not None:                   # (an empty selection is still a selection: any non-null pointer)
            sp = ctypes.c_void_p(sel.ctypes.data) if k else ctypes.c_void_p(ctypes.addressof(n))
        cap = 0 if cap is None else max(int(cap), 0)
        for _ in range(2):
            rows, info = np.zeros(cap, dtype=DECODED_DTYPE), np.zeros(cap, dtype=MERGED_DTYPE)
            rc = self.lib.adsb_stream_planes_merged(self._h, sp, k, cut, ctypes.c_void_p(rows.ctypes.data) if cap else None,
                                                    ctypes.c_void_p(info.ctypes.data) if cap else None, cap, ctypes.byref(n))
            if rc != -28:
                break
            cap = n.value
        self._chk(rc)
        return rows[:n.value], info[:n.value]

    def _n_streams(self):
        return getattr(self, "_streams_open", 0)

    def submit_format_host(self, fmt, data, abs_offset=0):
        """Host-fed pipelined submission (adsb_submit_format_host): data = host array in the format's layout; a
        page-locked one (PinnedArray, torch pin_memory) is DMA'd where it lies and must stay alive until wait()."""
        dt, per = FMT_LAYOUT[int(fmt)]
        data = np.ascontiguousarray(data, dtype=dt)
        t = ctypes.c_int32(-1)
        self._chk(self.lib.adsb_submit_format_host(self._h, int(fmt), ctypes.c_void_p(data.ctypes.data), len(data) // per,
                                                   int(abs_offset), ctypes.byref(t)))
        self._host_keepalive = getattr(self, "_host_keepalive", {})
        self._host_keepalive[t.value] = data
        return t.value

    def process_iq(self, iq, abs_offset=0):
        return self._host(FMT_FC32, iq, abs_offset)

    def process_mag2(self, x, abs_offset=0):
        return self._host(FMT_MAG2, x, abs_offset)

    def set_format_scale(self, fmt, scale):
        self._chk(self.lib.adsb_set_format_scale(self._h, int(fmt), float(np.float32(scale))))

    def process_format(self, fmt, data, abs_offset=0):
        """Host array in any ADSB_FMT_* layout (integer IQ: flat interleaved I,Q array of 2n items)."""
        return self._host(int(fmt), data, abs_offset)

    def process_format_device(self, fmt, dev_ptr, n, abs_offset=0, fetch=True):
        return self._device(int(fmt), dev_ptr, n, abs_offset, fetch)

    def _batch(self, fn, fmt, ptrs, ns, thresholds, abs_offsets):
        k = len(ptrs)
        items = np.zeros(k, dtype=BATCH_ITEM_DTYPE)
        items["data"] = np.asarray(ptrs, dtype=np.uint64)
        items["n"] = np.asarray(ns, dtype=np.int64)
        items["abs_offset"] = 0 if abs_offsets is None else np.asarray(abs_offsets, dtype=np.int64)
        items["threshold"] = self._thr if thresholds is None else np.asarray(thresholds, dtype=np.float32)
        first = np.zeros(k + 1, dtype=np.int32)
        n_out, n_fb = ctypes.c_int32(0), ctypes.c_int32(0)
        cap = getattr(self, "_batch_cap", 1 << 16)
        while True:
            out = np.empty(cap, dtype=BURST_DTYPE)
            rc = fn(self._h, int(fmt), ctypes.c_void_p(items.ctypes.data), k, ctypes.c_void_p(out.ctypes.data), cap,
                    ctypes.c_void_p(first.ctypes.data), ctypes.byref(n_out), ctypes.byref(n_fb))
            if rc == -28 and n_out.value > cap:          # -ENOSPC: *n_out = the number needed
                cap = self._batch_cap = n_out.value + n_out.value // 4
                continue
            self._chk(rc)
            break
        self.last_batch_fallbacks = n_fb.value
        return out[:n_out.value].copy(), first

    def process_batch_device(self, fmt, ptrs, ns, thresholds=None, abs_offsets=None):
        """Many independent streams in one device pass (adsb_process_batch_device): ptrs[i] = 16-byte aligned device pointer
        of item i, ns[i] its samples; thresholds[i] its framer threshold (None: the context's for every item); abs_offsets[i]
        the stream offset of its sample 0 (None: 0).  Returns (records, item_first): item i's records -- exactly those of
        process_format_device over the item alone -- are records[item_first[i]:item_first[i+1]].  last_batch_fallbacks =
        items that took the ordinary pass inside the call (longer than BATCH_ITEM_MAX, or a list overflow)."""
        return self._batch(self.lib.adsb_process_batch_device, fmt, [int(p) for p in ptrs], ns, thresholds, abs_offsets)

    def process_batch(self, fmt, arrays, thresholds=None, abs_offsets=None):
        """The same for host arrays in the format's layout (adsb_process_batch): pageable numpy arrays, or page-locked ones
        (PinnedArray.array, torch pin_memory), which are DMA'd where they lie.  Every array must start on a 16-byte boundary."""
        dt, per = FMT_LAYOUT[int(fmt)]
        arrays = [np.ascontiguousarray(a, dtype=dt) for a in arrays]
        for k, a in enumerate(arrays):
            if a.ctypes.data & 15:                       # a view into a larger array: the library wants 16-byte aligned items
                buf = np.empty(a.nbytes + 16, dtype=np.uint8)
                o = (-buf.ctypes.data) & 15
                arrays[k] = buf[o:o + a.nbytes].view(dt)
                arrays[k][...] = a
        return self._batch(self.lib.adsb_process_batch, fmt, [a.ctypes.data for a in arrays], [len(a) // per for a in arrays],
                           thresholds, abs_offsets)

    # Receiver streams carried across batch calls (adsb_process_stream_batch*; include/adsb_hip.h has the contract)
    def open_streams(self, n_streams):
        self._chk(self.lib.adsb_streams_open(self._h, int(n_streams)))
        self._streams_open = int(n_streams)

    def close_streams(self):
        self._chk(self.lib.adsb_streams_close(self._h))
        self._streams_open = 0

    def set_stream_base(self, stream, abs_offset):
        self._chk(self.lib.adsb_stream_set_base(self._h, int(stream), int(abs_offset)))

    def stream_state(self, stream):
        """(pos, eob, n_overlong): samples consumed, the carried end-of-burst offset (STREAM_FRESH_EOB on a fresh stream),
        pulses / bursts left out because they ran past a call's buffer"""
        p, e, o = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._chk(self.lib.adsb_stream_state(self._h, int(stream), ctypes.byref(p), ctypes.byref(e), ctypes.byref(o)))
        return p.value, e.value, o.value

    def reset_stream(self, stream):
        self._chk(self.lib.adsb_stream_reset(self._h, int(stream)))

    # FLAG_STREAM_DECODE contexts: one decoder behind every stream (include/adsb_hip.h STREAM DECODERS)
    def set_streams_decoder(self, msg_filter="All Messages"):
        """The msg_filter of every stream's decoder (adsb_streams_set_decoder)."""
        self._chk(self.lib.adsb_streams_set_decoder(self._h, DEC_MSG_FILTERS[msg_filter]))

    def set_stream_start(self, stream, start_timestamp):
        """The start timestamp of a fresh stream: a record's PDU timestamp is start + offset / fs (adsb_stream_set_start)."""
        self._chk(self.lib.adsb_stream_set_start(self._h, int(stream), float(start_timestamp)))

    def last_stream_decoded(self, copy=True):
        """DECODED_DTYPE rows of the last delivered stream-batch call: row t belongs to its record t (adsb_stream_last_decoded)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_stream_last_decoded(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=DECODED_DTYPE)
        buf = (ctypes.c_char * (n.value * DECODED_DTYPE.itemsize)).from_address(p.value)
        v = np.frombuffer(buf, dtype=DECODED_DTYPE)
        return v.copy() if copy else v

    # FLAG_STREAM_DECODE_SHARED contexts: one decoder behind all streams (include/adsb_hip.h SHARED DECODER)
    def last_stream_order(self):
        """int32[n]: the list position of the r-th record in the publication order -- ascending (timestamp, list position) --
        of the last delivered stream-batch call (adsb_stream_last_order)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_stream_last_order(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32)
        return np.frombuffer((ctypes.c_char * (n.value * 4)).from_address(p.value), dtype=np.int32).copy()

    def reset_streams_decoder(self):
        """A fresh shared decoder; the streams' framing state stays (adsb_streams_decoder_reset)."""
        self._chk(self.lib.adsb_streams_decoder_reset(self._h))

    # FLAG_STREAM_DEDUP contexts (include/adsb_hip.h DE-DUPLICATION)
    def set_streams_dedup(self, window_s=0.002, horizon_s=1.0):
        """The rule's window and the carry's horizon, in seconds, before the first delivered call (adsb_streams_set_dedup)."""
        self._chk(self.lib.adsb_streams_set_dedup(self._h, float(window_s), float(horizon_s)))

    def last_stream_duplicates(self):
        """int32[n] for the last delivered stream-batch call: -1 position t is no duplicate, -2 its match lies in an earlier
        call, else the list position of the earliest-published match of this call (adsb_stream_last_duplicates)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_stream_last_duplicates(self._h, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32)
        return np.frombuffer((ctypes.c_char * (n.value * 4)).from_address(p.value), dtype=np.int32).copy()

    def stream_dedup_stats(self):
        """(duplicates since the decoder was fresh, entries the carry holds, hi: the largest delivered timestamp)"""
        d, k, h = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0)
        self._chk(self.lib.adsb_stream_dedup_stats(self._h, ctypes.byref(d), ctypes.byref(k), ctypes.byref(h)))
        return d.value, k.value, h.value

    # multilateration on the de-duplication carry (include/adsb_hip.h MULTILATERATION)
    def set_stream_ecef(self, stream, x, y, z):
        """The antenna of `stream` in WGS-84 ECEF metres (adsb_stream_set_ecef); geodetic_to_ecef converts."""
        self._chk(self.lib.adsb_stream_set_ecef(self._h, int(stream), float(x), float(y), float(z)))

    def stream_mlat(self, t_lo=-np.inf, t_hi=np.inf, min_rx=4, cap=0, member_cap=0):
        """-> (fixes: MLAT_DTYPE[n], member_stream: int32[m], member_ts: float64[m]) for the groups of the carry whose head has
        t_lo <= ts < t_hi and at least min_rx used hearings (adsb_stream_mlat).  The call is repeated once with the capacity
        it asks for after -ENOSPC; cap / member_cap: where to start."""
        cap, member_cap = int(cap), int(member_cap)
        n, m = ctypes.c_int32(0), ctypes.c_int32(0)
        for attempt in (0, 1):
            fixes = np.zeros(cap, dtype=MLAT_DTYPE)
            ms, mt = np.zeros(member_cap, dtype=np.int32), np.zeros(member_cap, dtype=np.float64)
            rc = self.lib.adsb_stream_mlat(self._h, float(t_lo), float(t_hi), int(min_rx), fixes.ctypes.data if cap else None, cap,
                                           ctypes.byref(n), ms.ctypes.data if member_cap else None,
                                           mt.ctypes.data if member_cap else None, member_cap, ctypes.byref(m))
            if rc == -28 and attempt == 0:               # -ENOSPC: *n_fixes, *n_members = the numbers needed
                cap, member_cap = max(cap, n.value), max(member_cap, m.value)
                continue
            self._chk(rc)
            return fixes[:n.value], ms[:m.value], mt[:m.value]

    def stream_mlat_rule(self, rule, t_lo=-np.inf, t_hi=np.inf, cap=0, member_cap=0):
        """stream_mlat with the rule stated by the caller (adsb_stream_mlat_rule; rule: MLAT_RULE) -> (fixes: MLAT_DTYPE[n],
        aux: MLAT_AUX_DTYPE[n], member_stream, member_ts).  Asks once more after -ENOSPC, as stream_mlat does."""
        cap, member_cap = int(cap), int(member_cap)
        n, m = ctypes.c_int32(0), ctypes.c_int32(0)
        for attempt in (0, 1):
            fixes, aux = np.zeros(cap, dtype=MLAT_DTYPE), np.zeros(cap, dtype=MLAT_AUX_DTYPE)
            ms, mt = np.zeros(member_cap, dtype=np.int32), np.zeros(member_cap, dtype=np.float64)
            rc = self.lib.adsb_stream_mlat_rule(self._h, float(t_lo), float(t_hi), ctypes.byref(rule), fixes.ctypes.data if cap else None,
                                                aux.ctypes.data if cap else None, cap, ctypes.byref(n), ms.ctypes.data if member_cap else None,
                                                mt.ctypes.data if member_cap else None, member_cap, ctypes.byref(m))
            if rc == -28 and attempt == 0:
                cap, member_cap = max(cap, n.value), max(member_cap, m.value)
                continue
            self._chk(rc)
            return fixes[:n.value], aux[:n.value], ms[:m.value], mt[:m.value]

    def stream_mlat_stats(self):
        """(streams with a position, ts_ulp_m: what the double's spacing at the carry's latest timestamp is worth in metres)"""
        k, u = ctypes.c_int32(0), ctypes.c_double(0)
        self._chk(self.lib.adsb_stream_mlat_stats(self._h, ctypes.byref(k), ctypes.byref(u)))
        return k.value, u.value

    # the MLAT track store (include/adsb_hip.h MLAT TRACKS)
    def stream_mlat_track(self, rule, track_rule, t_lo=-np.inf, t_hi=np.inf):
        """One update of the device-side track store from the fixes adsb_stream_mlat_rule(rule) would return for [t_lo, t_hi)
        (adsb_stream_mlat_track; rule: MLAT_RULE, track_rule: MLAT_TRACK_RULE) -> the call's totals as a dict (MLAT_TRACK_STATS'
        fields).  No fix comes down."""
        st = MLAT_TRACK_STATS()
        self._chk(self.lib.adsb_stream_mlat_track(self._h, float(t_lo), float(t_hi), ctypes.byref(rule), ctypes.byref(track_rule), ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in MLAT_TRACK_STATS._fields_}

    def stream_mlat_tracks(self, min_fixes=1, cutoff=-np.inf, cap=None):
        """-> MLAT_TRACK_DTYPE[n]: the tracks with n_fixes >= min_fixes and last_ts >= cutoff, in ascending icao
        (adsb_stream_mlat_tracks).  cap None: a count query first; a cap that is too small is asked again with what is needed."""
        n = ctypes.c_int32(0)
        cap = 0 if cap is None else int(cap)
        for attempt in (0, 1):
            rows = np.zeros(cap, dtype=MLAT_TRACK_DTYPE)
            rc = self.lib.adsb_stream_mlat_tracks(self._h, int(min_fixes), float(cutoff), rows.ctypes.data if cap else None, cap, ctypes.byref(n))
            if rc == -28 and attempt == 0:
                cap = max(cap, n.value)
                continue
            self._chk(rc)
            return rows[:n.value]

    def expire_mlat_tracks(self, cutoff):
        """Removes the tracks with last_ts < cutoff (adsb_stream_mlat_tracks_expire) -> their number."""
        k = ctypes.c_int64(0)
        self._chk(self.lib.adsb_stream_mlat_tracks_expire(self._h, float(cutoff), ctypes.byref(k)))
        return k.value

    def reset_mlat_tracks(self):
        """Forgets every track (adsb_stream_mlat_tracks_reset)."""
        self._chk(self.lib.adsb_stream_mlat_tracks_reset(self._h))

    def stream_decoder_reserve(self, slots):
        """The capacity of the decoders' store, while it holds nothing (adsb_stream_decoder_reserve)."""
        self._chk(self.lib.adsb_stream_decoder_reserve(self._h, int(slots)))

    def stream_decoder_stats(self):
        """(planes of all streams together, slots of the store, growths since open_streams)"""
        p, c_, g = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._chk(self.lib.adsb_stream_decoder_stats(self._h, ctypes.byref(p), ctypes.byref(c_), ctypes.byref(g)))
        return p.value, c_.value, g.value

    def _stream_batch(self, fn, fmt, ids, ptrs, ns, thresholds, end, cap=None):
        k = len(ids)
        items = np.zeros(k, dtype=STREAM_ITEM_DTYPE)
        items["data"] = np.asarray(ptrs, dtype=np.uint64)
        items["n"] = np.asarray(ns, dtype=np.int64)
        items["stream"] = np.asarray(ids, dtype=np.int32)
        items["flags"] = np.where(np.broadcast_to(np.asarray(end, dtype=bool), (k,)), STREAM_END, 0)
        items["threshold"] = self._thr if thresholds is None else np.asarray(thresholds, dtype=np.float32)
        first = np.zeros(k + 1, dtype=np.int32)
        n_out, n_fb = ctypes.c_int32(0), ctypes.c_int32(0)
        fixed = cap is not None
        cap = cap if fixed else getattr(self, "_batch_cap", 1 << 16)
        while True:
            out = np.empty(cap, dtype=BURST_DTYPE)
            rc = fn(self._h, int(fmt), ctypes.c_void_p(items.ctypes.data), k, ctypes.c_void_p(out.ctypes.data), cap,
                    ctypes.c_void_p(first.ctypes.data), ctypes.byref(n_out), ctypes.byref(n_fb))
            if rc == -28 and n_out.value > cap and not fixed:      # -ENOSPC: no stream has moved, the call is repeated
                cap = self._batch_cap = n_out.value + n_out.value // 4
                continue
            self.last_stream_needed = n_out.value
            self._chk(rc)
            break
        self.last_batch_fallbacks = n_fb.value
        return out[:n_out.value].copy(), first

    def process_stream_batch_device(self, fmt, ids, ptrs, ns, thresholds=None, end=False, cap=None):
        """The next chunk of streams ids[i] in one device pass (adsb_process_stream_batch_device): ptrs[i] = device pointer
        (aligned to a sample) of ns[i] new samples; end: bool or one per item (STREAM_END).  Returns (records, item_first).
        cap: a fixed output capacity (the call raises AdsbError -ENOSPC instead of growing it; last_stream_needed = the
        number of records needed)."""
        return self._stream_batch(self.lib.adsb_process_stream_batch_device, fmt, ids, [int(p) for p in ptrs], ns, thresholds, end, cap)

    def process_stream_batch(self, fmt, ids, arrays, thresholds=None, end=False, cap=None):
        """The same for host arrays in the format's layout, any length and alignment (adsb_process_stream_batch)."""
        dt, per = FMT_LAYOUT[int(fmt)]
        arrays = [np.ascontiguousarray(a, dtype=dt) for a in arrays]
        return self._stream_batch(self.lib.adsb_process_stream_batch, fmt, ids, [a.ctypes.data for a in arrays],
                                  [len(a) // per for a in arrays], thresholds, end, cap)

    def submit_format_device(self, fmt, dev_ptr, n, abs_offset=0):
        return self._submit(int(fmt), dev_ptr, n, abs_offset)

    def set_iq16_scale(self, scale):
        self.set_format_scale(FMT_SC16, scale)

    def process_iq16(self, iq16, abs_offset=0):
        """iq16: int16 array of interleaved I,Q (2n shorts)."""
        return self._host(FMT_SC16, iq16, abs_offset)

    def process_iq16_device(self, dev_ptr, n, abs_offset=0, fetch=True):
        return self._device(FMT_SC16, dev_ptr, n, abs_offset, fetch)

    def submit_iq16_device(self, dev_ptr, n, abs_offset=0):
        return self._submit(FMT_SC16, dev_ptr, n, abs_offset)

    def process_iq_device(self, dev_ptr, n, abs_offset=0, fetch=True):
        return self._device(FMT_FC32, dev_ptr, n, abs_offset, fetch)

    def process_mag2_device(self, dev_ptr, n, abs_offset=0, fetch=True):
        return self._device(FMT_MAG2, dev_ptr, n, abs_offset, fetch)

    def submit_iq_device(self, dev_ptr, n, abs_offset=0):
        return self._submit(FMT_FC32, dev_ptr, n, abs_offset)

    def submit_mag2_device(self, dev_ptr, n, abs_offset=0):
        return self._submit(FMT_MAG2, dev_ptr, n, abs_offset)

    def submit_shard_device(self, fmt, dev_ptr, n, origin, own_lo, own_hi, stream_len, head_cands=0):
        t = ctypes.c_int32(-1)
        self._chk(self.lib.adsb_submit_shard_device(self._h, int(fmt), ctypes.c_void_p(int(dev_ptr)), int(n), int(origin),
                                                    int(own_lo), int(own_hi), int(stream_len), int(head_cands), ctypes.byref(t)))
        return t.value

    def wait(self, ticket, fetch=True, copy=True):
        n_out = ctypes.c_int32(0)
        try:
            self._chk(self.lib.adsb_wait(self._h, int(ticket), None, 0, ctypes.byref(n_out)))
        finally:
            # the host buffer of a host-fed submission was only kept alive for the upload: let go of it now, also on error
            getattr(self, "_host_keepalive", {}).pop(int(ticket), None)
        return self.last_result(copy=copy) if fetch else n_out.value

    def set_copy_threads(self, threads):
        """Host threads copying pageable host-fed sources into the pinned ring (before the first such submission)."""
        self._chk(self.lib.adsb_set_copy_threads(self._h, int(threads)))

    def host_copy(self, dst, src):
        """dst[:] = src for two contiguous host arrays of equal size, split over the context's copy threads."""
        assert dst.nbytes == src.nbytes and dst.flags.c_contiguous and src.flags.c_contiguous
        self._chk(self.lib.adsb_host_copy(self._h, ctypes.c_void_p(dst.ctypes.data), ctypes.c_void_p(src.ctypes.data), dst.nbytes))

    def wait_for_event(self, hip_event):
        """Everything submitted next runs after this hipEvent_t (raw handle) has completed: device-side ordering."""
        self._chk(self.lib.adsb_wait_for_event(self._h, ctypes.c_void_p(int(hip_event))))

    def clear_pending_events(self):
        self._chk(self.lib.adsb_clear_pending_events(self._h))

    def device_alloc(self, nbytes):
        """Device memory on this context's device (adsb_device_alloc) -> raw pointer; device_free it."""
        d = ctypes.c_void_p()
        self._chk(self.lib.adsb_device_alloc(self._h, ctypes.byref(d), int(nbytes)))
        return int(d.value)

    def device_free(self, dev_ptr):
        self._chk(self.lib.adsb_device_free(self._h, ctypes.c_void_p(int(dev_ptr))))

    def device_upload(self, dev_ptr, data):
        data = np.ascontiguousarray(data)
        self._chk(self.lib.adsb_device_upload(self._h, ctypes.c_void_p(int(dev_ptr)), ctypes.c_void_p(data.ctypes.data), data.nbytes))

    def framer_state(self):
        """(prev_in0, prev_eob_idx): the reference framer's cross-call attributes (framer.py:54,57)."""
        p, e = ctypes.c_float(0), ctypes.c_int64(0)
        self._chk(self.lib.adsb_framer_state(self._h, ctypes.byref(p), ctypes.byref(e)))
        return np.float32(p.value), int(e.value)

    def framer_work(self, in0, N, nitems_written, out0=None):
        """out0 (optional): the block's pass-through output, float32[N], contiguous -- filled by the library beside the device
        pass (adsb_framer_work_passthrough)."""
        if in0.dtype != np.float32 or not in0.flags.c_contiguous:
            in0 = np.ascontiguousarray(in0, dtype=np.float32)
        buf = getattr(self, "_tag_buf", None)
        if buf is None:
            buf = self._tag_buf = np.zeros(512, dtype=BURST_DTYPE)     # tags of one work() call, filled by the library
            self._tag_n = ctypes.c_int32(0)
            self._tag_ptr = ctypes.c_void_p(buf.ctypes.data)
        if out0 is not None:
            assert out0.dtype == np.float32 and out0.flags.c_contiguous and len(out0) == N
            rc = self.lib.adsb_framer_work_passthrough(self._h, ctypes.c_void_p(in0.ctypes.data), len(in0), int(N), int(nitems_written),
                                                       ctypes.c_void_p(out0.ctypes.data), self._tag_ptr, len(buf), ctypes.byref(self._tag_n))
        else:
            rc = self.lib.adsb_framer_work(self._h, ctypes.c_void_p(in0.ctypes.data), len(in0), int(N), int(nitems_written),
                                           self._tag_ptr, len(buf), ctypes.byref(self._tag_n))
        if rc == -28:                                                  # -ENOSPC: more tags than the buffer holds
            return self.last_result()
        self._chk(rc)
        return buf[:self._tag_n.value].copy()

    def demod_work(self, in0, nitems_read, tag_offsets, want_ratio=False):
        in0 = np.ascontiguousarray(in0, dtype=np.float32)
        tags = np.ascontiguousarray(tag_offsets, dtype=np.int64)
        nt = len(tags)
        bits = np.zeros((nt, 112), dtype=np.uint8)
        ok = np.zeros(nt, dtype=np.uint8)
        ratio = np.zeros((nt, 112), dtype=np.float32) if want_ratio else None
        self._chk(self.lib.adsb_demod_work(self._h, ctypes.c_void_p(in0.ctypes.data), len(in0), int(nitems_read),
                                           ctypes.c_void_p(tags.ctypes.data), nt, ctypes.c_void_p(bits.ctypes.data),
                                           ctypes.c_void_p(ok.ctypes.data),
                                           ctypes.c_void_p(ratio.ctypes.data) if want_ratio else None))
        self.last_demod_flags = ok        # ok[t] = BURST_DEMOD | parity pre-filter bits (0 = dropped); see demod_flags
        return bits, ok.astype(bool), ratio

    def process_sharded_device(self, fmt, dev_ptr, n, shards, abs_offset=0, out=None):
        """The resident stream as `shards` overlapped time shards, pipelined and stitched inside the library (one C call:
        adsb_process_sharded_device); bit-identical to process_format_device over the whole buffer.  out: a BURST_DTYPE array
        to receive the records (reused by callers that repeat the call); grown and retried when too small."""
        if out is None:
            out = np.empty(max(4096, int(n) // 4096), dtype=BURST_DTYPE)
        while True:
            n_out = ctypes.c_int32(0)
            rc = self.lib.adsb_process_sharded_device(self._h, int(fmt), ctypes.c_void_p(int(dev_ptr)), int(n), int(abs_offset),
                                                      int(shards), out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(n_out))
            if rc == -errno.ENOSPC and n_out.value > len(out):
                out = np.empty(n_out.value + n_out.value // 8 + 16, dtype=BURST_DTYPE)
                continue
            self._chk(rc)
            return out[:n_out.value]

    def shard_device(self, fmt, dev_ptr, n, origin, own_lo, own_hi, stream_len, head_cands=0):
        n_out = ctypes.c_int32(0)
        self._chk(self.lib.adsb_shard_device(self._h, int(fmt), ctypes.c_void_p(int(dev_ptr)), int(n), int(origin), int(own_lo),
                                             int(own_hi), int(stream_len), int(head_cands), None, 0, ctypes.byref(n_out)))
        return self.last_result()

    def shard_host(self, fmt, data, origin, own_lo, own_hi, stream_len, head_cands=0, drop_overlong=False):
        """adsb_shard_host: data = host array in the format's layout (see FMT_LAYOUT)."""
        dt, per = FMT_LAYOUT[int(fmt)]
        data = np.ascontiguousarray(data, dtype=dt)
        n_out = ctypes.c_int32(0)
        self._chk(self.lib.adsb_shard_host(self._h, int(fmt), ctypes.c_void_p(data.ctypes.data), len(data) // per, int(origin),
                                           int(own_lo), int(own_hi), int(stream_len), int(head_cands),
                                           SHARD_DROP_OVERLONG if drop_overlong else 0, None, 0, ctypes.byref(n_out)))
        return self.last_result()

    def stats(self):
        s = Stats()
        self._chk(self.lib.adsb_get_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def reset_stats(self):
        self._chk(self.lib.adsb_reset_stats(self._h))

    def numa_info(self):
        """{"node": NUMA node of the GPU's PCI device (-1 unknown / not bound), "cpulist": cpus local to it, "pci": address}."""
        node = ctypes.c_int32(-1)
        cl, bdf = ctypes.create_string_buffer(256), ctypes.create_string_buffer(32)
        self._chk(self.lib.adsb_numa_info(self._h, ctypes.byref(node), cl, len(cl), bdf, len(bdf)))
        return {"node": int(node.value), "cpulist": cl.value.decode(), "pci": bdf.value.decode()}

    def detect_history(self):
        """Per-launch k_detect durations (ms) since the last reset_stats, oldest first (FLAG_TIMING contexts)."""
        buf = np.zeros(4096, dtype=np.float32)
        n = ctypes.c_int32(0)
        self._chk(self.lib.adsb_detect_history(self._h, ctypes.c_void_p(buf.ctypes.data), len(buf), ctypes.byref(n)))
        return buf[:n.value].copy()


class PinnedArray:
    """NumPy view of page-locked host memory from adsb_host_alloc (freed when this object dies); with `near=ctx` on the
    NUMA node of that context's GPU (adsb_host_alloc_near)."""

    def __init__(self, n, dtype, near=None):
        self.lib = load()
        self.dtype = np.dtype(dtype)
        self.nbytes = int(n) * self.dtype.itemsize
        self._p = ctypes.c_void_p()
        if near is not None:
            rc = self.lib.adsb_host_alloc_near(near._h, ctypes.byref(self._p), max(1, self.nbytes))
        else:
            rc = self.lib.adsb_host_alloc(ctypes.byref(self._p), max(1, self.nbytes))
        if rc != 0:
            raise AdsbError(rc, "adsb_host_alloc")
        buf = (ctypes.c_char * max(1, self.nbytes)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(n))

    def __del__(self):
        try:
            if self._p.value:
                self.lib.adsb_host_free(self._p)
                self._p = ctypes.c_void_p()
        except Exception:
            pass


class RegisteredArray:
    """Page-locks an existing NumPy array in place (adsb_host_register) for as long as this object lives, so that
    host-fed submissions DMA it where it lies.  `with RegisteredArray(a): ...` or keep the object around."""

    def __init__(self, array):
        self.lib = load()
        self.array = np.ascontiguousarray(array)
        assert self.array is array or self.array.base is array or np.shares_memory(self.array, array), "array must be contiguous"
        rc = self.lib.adsb_host_register(ctypes.c_void_p(self.array.ctypes.data), self.array.nbytes)
        if rc != 0:
            raise AdsbError(rc, "adsb_host_register")
        self._live = True

    def close(self):
        if getattr(self, "_live", False):
            self.lib.adsb_host_unregister(ctypes.c_void_p(self.array.ctypes.data))
            self._live = False

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def process_sharded_multi(contexts, fmt, data, shards_per_ctx=1, abs_offset=0, out=None, want_stats=False):
    """ONE host buffer, N contexts (normally one per device), one stitched burst list: adsb_process_sharded_multi.  data =
    host array in the format's layout (FMT_LAYOUT; a PinnedArray / RegisteredArray view is DMA'd where it lies).  Returns the
    records -- bit-identical to Context.process_format over the whole buffer -- and, with want_stats, the per-context
    timings of the call as a dict."""
    lib = load()
    dt, per = FMT_LAYOUT[int(fmt)]
    data = np.ascontiguousarray(data, dtype=dt)
    n = len(data) // per
    arr = (ctypes.c_void_p * len(contexts))(*[cx._h for cx in contexts])
    if out is None:
        out = np.empty(max(4096, n // 4096), dtype=BURST_DTYPE)
    st = MultiStats()
    while True:
        n_out = ctypes.c_int32(0)
        rc = lib.adsb_process_sharded_multi(arr, len(contexts), int(fmt), ctypes.c_void_p(data.ctypes.data), n, int(abs_offset),
                                            int(shards_per_ctx), out.ctypes.data_as(ctypes.c_void_p), len(out),
                                            ctypes.byref(n_out), ctypes.byref(st))
        if rc == -errno.ENOSPC and n_out.value > len(out):
            out = np.empty(n_out.value + n_out.value // 8 + 16, dtype=BURST_DTYPE)
            continue
        if rc != 0:
            raise AdsbError(rc, lib.adsb_last_error(contexts[0]._h).decode("utf-8", "replace") if contexts else "")
        recs = out[:n_out.value]
        if not want_stats:
            return recs
        k = st.contexts
        return recs, {"contexts": k, "shards": st.shards, "fallbacks": st.fallbacks, "wall_s": st.wall_s,
                      "feeder_s": list(st.feeder_s[:k]), "device": list(st.device[:k]), "numa_node": list(st.numa_node[:k])}


def stitch(cands, sps):
    """Host stitch of shard candidate lists (already concatenated in stream order)."""
    lib = load()
    cands = np.ascontiguousarray(cands, dtype=BURST_DTYPE).copy()
    nk = ctypes.c_int32(0)
    rc = lib.adsb_stitch(ctypes.c_void_p(cands.ctypes.data), len(cands), int(sps), ctypes.byref(nk))
    if rc != 0:
        raise AdsbError(rc, "adsb_stitch")
    return cands[:nk.value]


BURST_HEAD = 16
SHARD_DROP_OVERLONG = 1
STREAM_UNBOUNDED = 1 << 60     # stream_len of a stream whose end is not known yet
MAX_HEAD = 4096          # upper bound on head_cands callers use
EOB_NONE = -(1 << 60)


def shard_fixup(recs, sps, eob_in, inplace=False):
    """Exact kept list of a gated shard (adsb_shard_device head_cands > 0) given the previous shard's tail.
    Returns None when the head region was too short (-EAGAIN).  inplace=True compacts recs itself (e.g. a
    last_result(copy=False) view of the pinned buffer) instead of a copy."""
    lib = load()
    if not inplace:
        recs = np.ascontiguousarray(recs, dtype=BURST_DTYPE).copy()
    assert recs.dtype == BURST_DTYPE and recs.flags.c_contiguous
    nk = ctypes.c_int32(0)
    rc = lib.adsb_shard_fixup(ctypes.c_void_p(recs.ctypes.data), len(recs), int(sps), int(eob_in), ctypes.byref(nk))
    if rc == -11:
        return None
    if rc != 0:
        raise AdsbError(rc, "adsb_shard_fixup")
    return recs[:nk.value]


SYNC_ALWAYS = (1 << 62)


def gate_window(recs, sps):
    """Samples the re-trigger gate stays closed after each burst: 63*sps (framer.py:165), 119*sps for records a
    long-aware context flagged BURST_LONG_HINT."""
    return np.where((recs["flags"] & BURST_LONG_HINT) != 0, 119, 63).astype(np.int64) * int(sps)


def shard_head_sync(recs, sps):
    """The one number that tells every rank -- for ANY incoming eob -- whether this shard's fresh-state gate
    decisions (and therefore its fresh-state tail, shard_tail) are exact from some head centre on: the largest
    offset of a head-region centre that starts an independent chain, i.e. lies beyond the reach (offset + gate
    window) of every head centre before it (the first centre of a shard always does).  If that offset is beyond
    the incoming eob the centre is accepted by the true gate and by the fresh-state gate alike, both hold the
    same state from there on, adsb_shard_fixup succeeds and the tail published from the fresh-state gate is the
    true one.  SYNC_ALWAYS for a shard without any centre (its tail is EOB_NONE: the incoming state passes
    through).  A shard that lies ENTIRELY in its head region gets no special treatment: its own fix-up could not
    fail, but if all its chain heads are at or before the incoming eob its true tail depends on that eob and the
    fresh-state tail it published would be stale (round-1 bug: such shards returned SYNC_ALWAYS)."""
    if len(recs) == 0:
        return SYNC_ALWAYS
    fl = recs["flags"]
    nh = int(np.count_nonzero(fl[:MAX_HEAD] & BURST_HEAD))
    if nh == 0:
        return EOB_NONE
    off = recs["offset"][:nh]
    reach = np.maximum.accumulate(off + gate_window(recs[:nh], sps))      # how far the centres so far can hold the gate
    idx = np.flatnonzero(off[1:] > reach[:-1])
    return int(off[idx[-1] + 1]) if len(idx) else int(off[0])


def shard_tail(recs, sps):
    """End-of-burst state a gated shard hands to the next one."""
    fl = recs["flags"]
    for i in range(len(recs) - 1, -1, -1):          # behind the head region every record is KEPT: O(1) in practice
        if fl[i] & BURST_KEPT:
            return int(recs["offset"][i]) + int(gate_window(recs[i:i + 1], sps)[0])
    return EOB_NONE


def snr_db_c(peak, median):
    return load().adsb_snr_db(float(peak), float(median))


def burst_df(recs):
    """Downlink format of every record (decoder.py:551), from the device's pre-filter bits."""
    return (recs["flags"] >> BURST_DF_SHIFT) & 31


def parity_ok(recs):
    """True where the decoder's check_parity() will pass without an aircraft table (DF 11/17/18/19, syndrome 0)."""
    return (recs["flags"] & BURST_PARITY_OK) != 0


def shard_bounds(stream_len, n_shards, g, sps, align=4096):
    """adsb_shard_bounds: (own_lo, own_hi, lo, hi) of shard g (pure host arithmetic, no device needed)."""
    v = [ctypes.c_int64(0) for _ in range(4)]
    rc = load().adsb_shard_bounds(int(stream_len), int(n_shards), int(g), int(sps), int(align), *[ctypes.byref(x) for x in v])
    if rc:
        raise AdsbError(rc, "adsb_shard_bounds")
    return tuple(x.value for x in v)


def plan_chunks(n_samples, resident_wavefronts):
    """(units, samples_per_chunk) of one call over n_samples (adsb_plan_chunks: pure host arithmetic)."""
    u, t = ctypes.c_int64(), ctypes.c_int64()
    rc = load().adsb_plan_chunks(int(n_samples), int(resident_wavefronts), ctypes.byref(u), ctypes.byref(t))
    if rc != 0:
        raise AdsbError(rc, "adsb_plan_chunks")
    return u.value, t.value


def mode_s_syndrome(bits14):
    """(syndrome, df, nbits) of one 14-byte payload via the C helper: the announced address for the
    address/parity formats (decoder.py:577,647)."""
    b = np.ascontiguousarray(bits14, dtype=np.uint8)
    assert b.size == 14
    df, nb = ctypes.c_int32(), ctypes.c_int32()
    syn = load().adsb_mode_s_syndrome(b.ctypes.data_as(ctypes.c_void_p), ctypes.byref(df), ctypes.byref(nb))
    return int(syn), df.value, nb.value


def mode_s_fec(bits14):
    """adsb_mode_s_fec: (flags, repaired bits14, first_bit, nflip) of one 14-byte payload -- the rule FLAG_FEC_CONSERVATIVE
    applies on the device (flags: pre-filter bits of the result | BURST_FEC_FIXED or BURST_FEC_DF)."""
    b = np.ascontiguousarray(bits14, dtype=np.uint8)
    assert b.size == 14
    out = np.zeros(14, dtype=np.uint8)
    first, nflip = ctypes.c_int32(), ctypes.c_int32()
    fl = load().adsb_mode_s_fec(b.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(first),
                                ctypes.byref(nflip))
    return int(fl), out, first.value, nflip.value


def mode_s_soft_fec(bits14, key, n_weak=8, max_flips=3, min_key=0.0):
    """adsb_mode_s_soft_fec: (flags, repaired bits14, SOFT_DTYPE row) of one 14-byte payload and the weakness key[112] of its
    bits -- the rule FLAG_FEC_SOFT applies on the device (flags: pre-filter bits of the result | BURST_FEC_FIXED on a match)."""
    b = np.ascontiguousarray(bits14, dtype=np.uint8)
    k = np.ascontiguousarray(key, dtype=np.float32)
    assert b.size == 14 and k.size == 112
    out = np.zeros(14, dtype=np.uint8)
    row = np.zeros(1, dtype=SOFT_DTYPE)
    rule = SOFT_FEC_RULE(int(n_weak), int(max_flips), float(min_key), 0)
    fl = load().adsb_mode_s_soft_fec(b.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rule),
                                  out.ctypes.data_as(ctypes.c_void_p), row.ctypes.data_as(ctypes.c_void_p))
    return int(fl), out, row[0]


def mode_s_aircraft(bits14, fec=False):
    """adsb_mode_s_aircraft: (ap_fec, aa, announce, fec_announce) of one 14-byte payload -- the per-PDU rule FLAG_AIRCRAFT_TABLE
    applies on the device (aa: the AA of an address/parity reply or -1; announce: the address the PDU announces whatever the
    table holds, or -1; ap_fec: an unknown address/parity reply the Conservative repair accepts, then announcing
    fec_announce, or -1)."""
    b = np.ascontiguousarray(bits14, dtype=np.uint8)
    assert b.size == 14
    aa, ann, fann = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    r = load().adsb_mode_s_aircraft(b.ctypes.data_as(ctypes.c_void_p), 1 if fec else 0, ctypes.byref(aa), ctypes.byref(ann),
                                    ctypes.byref(fann))
    return bool(r & BURST_AP_FEC), aa.value, ann.value, fann.value


def demod_flags(ok):
    """adsb_demod_work's ok[] bytes -> the record flag layout (uint16): bits 0, 5-7 are the same, the FEC verdicts of an
    FLAG_FEC_CONSERVATIVE context travel in bits 1 / 2 (BURST_FEC_FIXED >> 13 / BURST_FEC_DF >> 13), the aircraft table's
    of a FLAG_AIRCRAFT_TABLE context in bits 3 / 4 (BURST_AP_KNOWN / BURST_AP_FEC << 2)."""
    ok = np.asarray(ok, dtype=np.uint16)
    return (ok & 0xE1) | ((ok & 6) << 13) | (ok & BURST_AP_KNOWN) | ((ok & 16) >> 2)


def unpack_bits(bits14):
    """[n,14] packed bytes -> [n,112] 0/1 uint8 (the u8vector layout of the reference PDU)."""
    return np.unpackbits(np.asarray(bits14, dtype=np.uint8).reshape(-1, 14), axis=1, bitorder="big")


def confidence_db(ratio):
    """demod.py:101: bit_confidence = 10*log10(bit1_amp / bit0_amp), float32 with NumPy itself (like snr_db)."""
    with np.errstate(all="ignore"):
        return (np.float32(10.0) * np.log10(np.asarray(ratio, dtype=np.float32))).astype(np.float32)


def snr_db(peak, median):
    """10*log10(peak/median)+1.6 in float32 with NumPy itself, so the bits equal the reference's
    (framer.py:157 under NumPy-2 promotion) on whatever host this runs on."""
    with np.errstate(all="ignore"):
        p = np.asarray(peak, dtype=np.float32)
        m = np.asarray(median, dtype=np.float32)
        return (np.float32(10.0) * np.log10(p / m) + np.float32(1.6)).astype(np.float32)


def decoded_pdu(row, meta):
    """One adsb_decoded row plus the incoming PDU's meta ({"timestamp", "snr", ...}) -> what the reference decoder publishes
    for it: ("decoded" | "unknown", (meta dict, u8vector of 112 bits)), or None when it publishes nothing (a raising PDU
    included).  Fields, types and key order as decoder.py:512-538 builds them: speed and heading from the integer velocity
    components with NumPy's sqrt and arctan2 (:1190-1191), NaN where the plane has no value, datetime from the timestamp."""
    import datetime
    port = int(row["port"])
    if port not in (DEC_DECODED, DEC_UNKNOWN):
        return None
    ts = meta["timestamp"]
    dt = datetime.datetime.utcfromtimestamp(ts).strftime("%Y-%m-%d %H:%M:%S.%f UTC")
    vec = unpack_bits(np.asarray(row["bits"], dtype=np.uint8)).reshape(112)
    if port == DEC_UNKNOWN:
        return "unknown", ({"timestamp": ts, "datetime": dt, "df": int(row["df"]), "snr": meta["snr"]}, vec)
    d = plane_entry(row)
    d["timestamp"] = ts
    d["datetime"] = dt
    d["icao"] = "{:06x}".format(int(row["icao"]))
    d["df"] = int(row["df"])
    d["snr"] = meta["snr"]
    return "decoded", (d, vec)


def check_stream_selection(streams, n_streams):
    """adsb_stream_planes' rule for a selection: indices in 0 .. n_streams - 1, strictly ascending (ValueError otherwise)."""
    sel = [int(x) for x in streams]
    if any(x < 0 or x >= n_streams for x in sel):
        raise ValueError("stream indices have to be in 0 .. %d: %r" % (n_streams - 1, sel))
    if any(b <= a for a, b in zip(sel, sel[1:])):
        raise ValueError("stream indices have to be strictly ascending: %r" % (sel,))


def plane_entry(row, last_seen=None):
    """One snapshot row (Context.planes / stream_planes) -> the reference's plane_dict entry (decoder.py:413-449) without
    "cpr" and "last_seen": callsign (None or str), altitude, speed, heading, vertical_rate, latitude, longitude, num_msgs,
    with decoded_pdu's conversions and Python types (speed and heading with NumPy from the integer components, NaN where the
    plane has no value).  last_seen (planes(seen=True)): the entry's "last_seen" too, an int behind num_msgs as the
    reference has it."""
    pr = int(row["present"])
    nan = float("nan")
    d = {"callsign": bytes(row["callsign"]).rstrip(b"\0").decode() if pr & DEC_HAS_CALLSIGN else None,
         "altitude": int(row["altitude"]) if pr & DEC_HAS_ALTITUDE else nan}
    if pr & DEC_HAS_VELOCITY:
        vwe, vsn = int(row["velocity_we"]), int(row["velocity_sn"])
        d["speed"] = np.sqrt(vsn**2 + vwe**2)
        d["heading"] = np.arctan2(vsn, vwe) * 360.0 / (2.0 * np.pi)
        d["vertical_rate"] = int(row["vertical_rate"])
    else:
        d["speed"] = d["heading"] = d["vertical_rate"] = nan
    d["latitude"] = float(row["latitude"])
    d["longitude"] = float(row["longitude"])
    d["num_msgs"] = int(row["num_msgs"])
    if last_seen is not None:
        d["last_seen"] = int(last_seen)
    return d


def plane_table(rows, timestamp):
    """The lines print_planes (decoder.py:455-506) draws for these snapshot rows at PDU timestamp `timestamp`: one string per
    plane, in the rows' order."""
    import datetime
    seen = datetime.datetime.utcfromtimestamp(timestamp).strftime("%H:%M:%S")
    out = []
    for row in rows:
        p = plane_entry(row)
        num = lambda v, f, w: f.format(v) if not np.isnan(v) else " " * w     # noqa: E731
        out.append("{:8s} {:6s} {} {} {} {} {} {} {} {}".format(
            seen, "{:06x}".format(int(row["icao"])),
            "{:8s}".format(p["callsign"]) if p["callsign"] is not None else " " * 8,
            num(p["altitude"], "{:5.0f}", 5), num(p["vertical_rate"], "{:5.0f}", 5), num(p["speed"], "{:5.0f}", 5),
            num(p["heading"], "{:5.0f}", 5), num(p["latitude"], "{:11.7f}", 11), num(p["longitude"], "{:11.7f}", 11),
            "{:4d}".format(p["num_msgs"])))
    return out
