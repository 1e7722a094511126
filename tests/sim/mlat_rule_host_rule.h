// mlat_rule_host_rule.h -- TEST INFRASTRUCTURE ONLY.  mlat_host_rule.h for adsb_stream_mlat_rule's damped path: what its two
// drivers -- tests/sim/mlat_rule_driver.cpp (the SIMT emulator) and tests/gpu/mlat_rule_device_driver.hip (the shipped units, on
// the GPU) -- restate of the host's rule in adsb_hip.hip, stated once for both: the parts of the work buffer adsb_mlat_rule.h's
// layout_rule() carves with the bytes a call may write, the argument table of the entry point, and the range check of the
// group counts (groups of three are possible: ng <= nc / 3).  Host code only; needs adsb_mlat_rule.h and mlat_host_rule.h.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

namespace mlat_rule {

constexpr int kSolverGn = 0, kSolverLm = 1, kRestart = 1, kAltitude = 2;

inline std::vector<std::pair<size_t, size_t>> parts_rule(const mh::RuleLayout& L, size_t nc, size_t n_streams) {
  const size_t chunks = (nc + mh::kChunk - 1) / mh::kChunk + 1;
  return {{L.range, 16}, {L.tot_heads, 16}, {L.tot_groups, 16}, {L.w, nc * 4}, {L.cnt, chunks * 4}, {L.sum, chunks * 4}, {L.heads, nc * 4},
          {L.nrx, nc * 4}, {L.gsel, nc * 4}, {L.gfirst, nc * 4}, {L.rx, n_streams * 24}, {L.fixes, mh::rule_rows(nc) * (size_t)mh::kFixBytes},
          {L.member_stream, nc * 4}, {L.member_ts, nc * 8}, {L.aux, mh::rule_rows(nc) * (size_t)mh::kAuxBytes}};
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

inline bool groups_in_range_rule(int ng, int nm, int nc, int min_rx) {
  return !(ng < 0 || ng > nc / mh::kMinRxAided || nm < (long long)ng * min_rx || nm > nc);
}

}  // namespace mlat_rule
