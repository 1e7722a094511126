// mlat_rule_host_rule.h -- TEST INFRASTRUCTURE ONLY.  mlat_host_rule.h for adsb_stream_mlat_rule's damped path: what its two
// drivers -- tests/sim/mlat_rule_driver.cpp (the SIMT emulator) and tests/gpu/mlat_rule_device_driver.hip (the shipped units, on
// the GPU) -- restate of the host's rule in adsb_hip.hip, stated once for both: the parts of the work buffer adsb_mlat_rule.h's
// layout_rule() carves with the bytes a call may write, and the argument table of the entry point.  (The range check of the
// group counts is mlat_host_rule.h's, with kMinRxAided: groups of three are possible.)  Host code only; needs adsb_mlat_rule.h
// and mlat_host_rule.h.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

namespace mlat_rule {

constexpr int kSolverGn = 0, kSolverLm = 1, kRestart = 1, kAltitude = 2;

inline std::vector<std::pair<size_t, size_t>> parts_rule(const mh::RuleLayout& L, size_t nc, size_t n_streams) {
  return parts(L, nc, n_streams, mh::rule_rows(nc), mh::kAuxBytes);
}

// adsb_stream_mlat_rule's argument table, with its own expressions -> true: -EINVAL
inline bool rule_refused(int solver, int flags, int min_rx, int reserved, double alt_weight) {
  if (solver != kSolverGn && solver != kSolverLm) return true;
  if (flags & ~(kRestart | kAltitude)) return true;
  if (solver == kSolverGn && flags != 0) return true;
  if (reserved != 0) return true;
  if (min_rx < ((flags & kAltitude) ? mh::kMinRxAided : mh::kMinRx)) return true;
  if ((flags & kAltitude) && !(alt_weight > 0.0 && alt_weight <= 1.7976931348623157e308)) return true;
  return false;
}

}  // namespace mlat_rule
