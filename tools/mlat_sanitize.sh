#!/bin/bash
# adsb_stream_mlat's device code (gr_adsb_amd/csrc/adsb_mlat_device.h) and the host's sizing rule (adsb_mlat.h: layout()) under
# AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, as a STAND-ALONE program: tests/sim/mlat_sanitize_main.cpp (the
# emulator driver tests/sim/mlat_driver.cpp and a main of its own) runs the sizing rule and two of tests/test_mlat.py's cases.
# Nothing sanitized is loaded into python.
#   bash tools/mlat_sanitize.sh            (CPU box; under a minute)
set -e
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O1 -g -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    tests/sim/mlat_sanitize_main.cpp -o "$TMP/mlat_sanitize"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 "$TMP/mlat_sanitize"
