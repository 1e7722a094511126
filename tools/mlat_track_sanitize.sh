#!/bin/bash
# The MLAT track store's device code (gr_adsb_amd/csrc/adsb_mlat_track_device.h), its real launchers and sizing rule
# (adsb_mlat_track.hip, adsb_mlat_track.h; adsb_shared.hip's launch_sort) and the drivers' host rule
# (tests/sim/mlat_track_host_rule.h) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, as a STAND-ALONE program:
# tests/sim/mlat_track_sanitize_main.cpp (the emulator driver tests/sim/mlat_track_driver.cpp and a main of its own) runs the
# sizing rule and tests/test_mlat_track.py's kinds of call.  Nothing sanitized is loaded into python.
#   bash tools/mlat_track_sanitize.sh       (CPU box; under a minute)
set -e
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O1 -g -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I tests/sim/hipstub tests/sim/mlat_track_sanitize_main.cpp -o "$TMP/mlat_track_sanitize"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 "$TMP/mlat_track_sanitize"
