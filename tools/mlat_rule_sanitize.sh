#!/bin/bash
# adsb_stream_mlat_rule's device code (gr_adsb_amd/csrc/adsb_mlat_rule_device.h on adsb_mlat_device.h) and the host's sizing rule
# (adsb_mlat_rule.h: layout_rule()) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, as a STAND-ALONE program:
# tests/sim/mlat_rule_sanitize_main.cpp (the emulator driver tests/sim/mlat_rule_driver.cpp and a main of its own) runs the
# sizing rule and tests/test_mlat_rule.py's kinds of call.  Nothing sanitized is loaded into python.
#   bash tools/mlat_rule_sanitize.sh       (CPU box; under a minute)
set -e
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O1 -g -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    tests/sim/mlat_rule_sanitize_main.cpp -o "$TMP/mlat_rule_sanitize"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 "$TMP/mlat_rule_sanitize"
