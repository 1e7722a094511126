// adsb_mlat_rule.h -- the launchers of adsb_mlat_rule.hip (adsb_stream_mlat_rule's damped solver: adsb_mlat_rule_device.h), for
// adsb_hip.hip, and the sizing rule of that call's work buffer.  Beside adsb_mlat.h, which stays as it is: the range, the heads
// and the compaction are its launch_heads and launch_select, on a RuleLayout (a Layout with other sizes and one more part).
// Plain pointers only; every call queues its kernels on `stream` and returns the hipError_t of the launches as an int.
// Internal to libadsb_hip.so.
#pragma once
#include <stddef.h>

#include "adsb_mlat.h"

namespace adsb_mlat_host {

constexpr int kAuxBytes = 32, kMinRxAided = 3;

// layout() for a call that may select groups of kMinRxAided used hearings: groups <= nc / 3, so fixes and aux hold nc / 3 + 1
// rows; everything else as layout() sizes it, aux behind member_ts.
struct RuleLayout : Layout {
  size_t aux;                             // Aux[nc / kMinRxAided + 1]
};
inline size_t rule_rows(size_t nc) { return nc / kMinRxAided + 1; }
inline RuleLayout layout_rule(size_t nc, size_t n_streams) {
  RuleLayout L{};
  const size_t chunks = (nc + kChunk - 1) / kChunk + 1;
  const size_t part[15] = {16, 16, 16, nc * 4, chunks * 4, chunks * 4, nc * 4, nc * 4, nc * 4, nc * 4, n_streams * 24,
                           rule_rows(nc) * (size_t)kFixBytes, nc * 4, nc * 8, rule_rows(nc) * (size_t)kAuxBytes};
  size_t* const at[15] = {&L.range, &L.tot_heads, &L.tot_groups, &L.w, &L.cnt, &L.sum, &L.heads, &L.nrx, &L.gsel, &L.gfirst, &L.rx,
                          &L.fixes, &L.member_stream, &L.member_ts, &L.aux};
  size_t off = 0;
  for (int k = 0; k < 15; ++k) { *at[k] = off; off += (part[k] + 255) & ~(size_t)255; }
  L.bytes = off;
  return L;
}

// heads[nh] -> nrx[nh], 0 for a three-hearing group without an altitude; then launch_select with min_rx
int launch_groups_rule(void* stream, const void* carry, int nc, int nh, double window, int min_rx, int n_streams, void* work, const RuleLayout& L);
// gsel[ng] -> fixes[ng], aux[ng], member_stream / member_ts by the damped rule; flags: ADSB_MLAT_RESTART | ADSB_MLAT_ALTITUDE
int launch_solve_lm(void* stream, const void* carry, int nc, int ng, double window, int n_streams, int flags, double alt_weight, void* work,
                    const RuleLayout& L);

}  // namespace adsb_mlat_host
