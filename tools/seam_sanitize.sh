#!/bin/bash
# The sharded drivers' seam consumer (gr_adsb_amd/csrc/adsb_seam.h) under AddressSanitizer + UndefinedBehaviorSanitizer on the
# CPU, as a STAND-ALONE program: tests/sim/seam_sanitize_main.cpp (the test driver tests/sim/seam_driver.cpp and a main of its
# own) runs it over generated worlds with output arrays from too small to large enough.  Nothing sanitized is loaded into python.
#   bash tools/seam_sanitize.sh            (CPU box; a few seconds)
set -e
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O1 -g -std=c++17 -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    tests/sim/seam_sanitize_main.cpp -o "$TMP/seam_sanitize"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 "$TMP/seam_sanitize"
