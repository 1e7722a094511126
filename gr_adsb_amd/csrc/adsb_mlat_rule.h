// adsb_mlat_rule.h -- the launchers of adsb_mlat_rule.hip (adsb_stream_mlat_rule's damped solver: adsb_mlat_rule_device.h), for
// adsb_hip.hip, and the sizing rule of that call's work buffer.  Beside adsb_mlat.h, which stays as it is: the range, the heads
// and the compaction are its launch_heads and launch_select, on a Layout carved with other row counts and the aux part.
// Plain pointers only; every call queues its kernels on `stream` and returns the hipError_t of the launches as an int.
// Internal to libadsb_hip.so.
#pragma once
#include <stddef.h>

#include "adsb_mlat.h"

namespace adsb_mlat_host {

constexpr int kAuxBytes = 32, kMinRxAided = 3;

// The work buffer of a call that may select groups of kMinRxAided used hearings: groups <= nc / 3, so fixes and aux hold
// nc / 3 + 1 rows; everything else as layout() sizes it.  RuleLayout: a Layout carved this way, aux part included.
using RuleLayout = Layout;
inline size_t rule_rows(size_t nc) { return nc / kMinRxAided + 1; }
inline RuleLayout layout_rule(size_t nc, size_t n_streams) { return carve(nc, n_streams, rule_rows(nc), kAuxBytes); }

// heads[nh] -> nrx[nh], 0 for a three-hearing group without an altitude; then launch_select with min_rx
int launch_groups_rule(void* stream, const void* carry, int nc, int nh, double window, int min_rx, int n_streams, void* work, const RuleLayout& L);
// gsel[ng] -> fixes[ng], aux[ng], member_stream / member_ts by the damped rule; flags: ADSB_MLAT_RESTART | ADSB_MLAT_ALTITUDE
int launch_solve_lm(void* stream, const void* carry, int nc, int ng, double window, int n_streams, int flags, double alt_weight, void* work,
                    const RuleLayout& L);

}  // namespace adsb_mlat_host
