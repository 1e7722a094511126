#!/bin/bash
# The shared decoder's device code (gr_adsb_amd/csrc/adsb_shared_device.h around adsb_device.h's k_fleet_*) under
# AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, as a STAND-ALONE program: tests/sim/shared_sanitize_main.cpp (the
# emulator driver tests/sim/shared_driver.cpp and a main of its own) drives the pair sort and one partition of
# tests/golden/g_shared.npz.  Nothing sanitized is loaded into python: python only writes the job file first.
#   bash tools/shared_sanitize.sh            (CPU box; under a minute)
set -e
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
python tools/shared_sanitize_job.py "$TMP/job.bin"
g++ -O1 -g -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    tests/sim/shared_sanitize_main.cpp -o "$TMP/shared_sanitize"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 "$TMP/shared_sanitize" "$TMP/job.bin"
