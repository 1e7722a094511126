#!/bin/bash
# The soft-decision CRC repair's shipped translation unit (gr_adsb_amd/csrc/adsb_softfec.hip: the host rule
# adsb_mode_s_soft_fec, the real launchers, and the kernels of adsb_softfec_device.h on the SIMT emulator) under AddressSanitizer +
# UndefinedBehaviorSanitizer on the CPU, as a STAND-ALONE program: tests/sim/softfec_sanitize_main.cpp has a main of its own and
# holds the emulated kernels' bytes against the host rule's.  Nothing sanitized is loaded into python.
#   bash tools/softfec_sanitize.sh       (CPU box; under a minute)
set -e
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O1 -g -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -I tests/sim/hipstub tests/sim/softfec_sanitize_main.cpp -o "$TMP/softfec_sanitize"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 "$TMP/softfec_sanitize"
