"""The MLAT track store's C ABI as the header states it, against its Python mirrors and the replay -- CPU only: struct sizes and
offsets, export names, constants, dtype field order, the Python layer's defaults, and the documents' side of the issue."""
import ctypes
import inspect
import os
import re

import numpy as np

import mlat_track_replay as R
from gr_adsb_amd import _native as N
from gr_adsb_amd import frontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
HDR = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
CALLS = ("adsb_stream_mlat_track", "adsb_stream_mlat_tracks", "adsb_stream_mlat_tracks_expire", "adsb_stream_mlat_tracks_reset")


def fields_of(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HDR, re.S).group(1)
    return re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_struct_sizes_and_offsets():
    assert ctypes.sizeof(N.MLAT_TRACK_RULE) == 64 and N.MLAT_TRACK_DTYPE.itemsize == 96 and ctypes.sizeof(N.MLAT_TRACK_STATS) == 64
    for struct, size in (("adsb_mlat_track_rule", 64), ("adsb_mlat_track", 96), ("adsb_mlat_track_stats", 64)):
        assert re.search(r"typedef struct %s \{ /\* %d bytes \*/" % (struct, size), HDR), struct
    rule = {name: getattr(N.MLAT_TRACK_RULE, name).offset for name, _ in N.MLAT_TRACK_RULE._fields_}
    assert rule == dict(alpha=0, beta=8, gate_m=16, max_speed_mps=24, max_gap_s=32, max_rms_m=40, min_up_m=48, restart_after=56, reserved=60)
    row = {name: N.MLAT_TRACK_DTYPE.fields[name][1] for name in N.MLAT_TRACK_DTYPE.names}
    assert row == dict(icao=0, flags=4, n_fixes=8, n_rejected=12, first_ts=16, last_ts=24, x=32, y=40, z=48, vx=56, vy=64, vz=72, rms_m=80, n_rx=88,
                       misses=92)
    assert N.MLAT_TRACK_DTYPE["flags"] == np.dtype("<u4") and N.MLAT_TRACK_DTYPE["icao"] == np.dtype("<i4")
    assert [getattr(N.MLAT_TRACK_STATS, name).offset for name, _ in N.MLAT_TRACK_STATS._fields_] == list(range(0, 64, 8))


def test_the_mirrors_have_the_headers_fields():
    assert fields_of("adsb_mlat_track_rule") == [name for name, _ in N.MLAT_TRACK_RULE._fields_]
    assert fields_of("adsb_mlat_track") == list(N.MLAT_TRACK_DTYPE.names)
    assert fields_of("adsb_mlat_track_stats") == [name for name, _ in N.MLAT_TRACK_STATS._fields_] == list(R.STATS)


def test_exports_constants_and_defaults():
    assert re.search(r"#define ADSB_ABI_VERSION (\d+)", HDR).group(1) == "5" and N.ABI_VERSION == 5
    for name in CALLS:
        assert name in N.EXPORTS and re.search(r"^int %s\(adsb_ctx\* ctx" % name, HDR, re.M), name
    for name, value in (("GAP", 1), ("RESTARTED", 2)):
        assert int(re.search(r"#define ADSB_TRACK_%s (\d+)u$" % name, HDR, re.M).group(1)) == getattr(N, "TRACK_" + name) == getattr(R, name) == value
    assert N.MLAT_TRACK_DEFAULTS == R.DEFAULTS == dict(alpha=0.3, beta=0.05, gate_m=2000.0, max_speed_mps=350.0, max_gap_s=30.0, restart_after=3,
                                                       max_rms_m=500.0, min_up_m=0.0)
    r = N.mlat_track_rule(gate_m=1.0, restart_after=7)
    assert (r.alpha, r.beta, r.gate_m, r.max_speed_mps, r.max_gap_s, r.max_rms_m, r.min_up_m, r.restart_after, r.reserved) == \
        (0.3, 0.05, 1.0, 350.0, 30.0, 500.0, 0.0, 7, 0)
    for name in ("stream_mlat_track", "stream_mlat_tracks", "expire_mlat_tracks", "reset_mlat_tracks"):
        assert callable(getattr(N.Context, name))
    sig = inspect.signature(N.Context.stream_mlat_tracks).parameters
    assert sig["min_fixes"].default == 1 and sig["cutoff"].default == -np.inf and sig["cap"].default is None
    sig = inspect.signature(frontend.Receivers.track).parameters
    assert (sig["solver"].default, sig["restart"].default, sig["altitude"].default, sig["alt_weight"].default, sig["min_rx"].default) == \
        ("damped", True, False, 1.0, 4)
    assert inspect.signature(frontend.Receivers.tracks).parameters["min_fixes"].default == 3
    assert inspect.signature(frontend.Receivers.merged).parameters["mlat"].default is False
    assert inspect.signature(frontend.Receivers.table).parameters["mlat"].default is False


def test_the_documents():
    assert "MLAT TRACKS" in HDR and all(w in HDR for w in ("USABLE", "STALE", "START", "GATE", "STEP", "LIMITS"))
    assert "not a Kalman filter" in HDR and "one simulation" in HDR.replace("\n * ", " ")
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (HDR, design):
        assert "feeding fixes into the plane table" not in text and "feeding MLAT fixes into the plane table" not in text
    assert "Sub-sample arrival times, clock offsets between receivers" in HDR and "sub-sample arrival times" in design
    assert "### 3j." in design and "hash table" in design.split("### 3j.")[1]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in CALLS:
        assert name in integration, name
    assert "adsb_stream_mlat_track" in readme and "mlat_track_cost" in readme
