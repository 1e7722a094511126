// mlat_track_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  The twin of tests/sim/mlat_track_driver.cpp on the GPU: the same
// entry points (sim_track_update, sim_track_read, sim_track_expire and the sizing exports) with the same arguments and return
// codes, over the SHIPPED translation unit gr_adsb_amd/csrc/adsb_mlat_track.hip -- compiled as a unit of its own with the
// library's flags and linked beside this file into tests/gpu/libadsb_mlat_track_dev.so (tests/test_gpu_mlat_track_device.py
// builds it with tests/device_build.py) -- and its real launchers with their own cover().  The unit's key sort is
// adsb_shared.hip's launch_sort; that shipped unit is compiled into this file's object as it stands, so the library holds the
// sort the unit calls.  The host's rule is tests/sim/mlat_track_host_rule.h, shared with the emulator driver; a Part is device
// memory with a guard tail (device_buffers.h), read back whole behind every launch group, and the first HIP error is sticky.
// This file launches no kernel of its own.  Never linked into libadsb_hip.so.
#include "device_buffers.h"

#include "../../gr_adsb_amd/csrc/adsb_shared.hip"

#include "../../gr_adsb_amd/csrc/adsb_mlat_track.h"
#include "../sim/mlat_track_host_rule.h"

namespace th = adsb_mlat_track_host;

static_assert(th::kRowBytes == 96 && th::kRuleBytes == 64 && track_rule::kGuardByte == kGuard, "the sizes adsb_mlat_track.h states");

extern "C" {

int dev_track_dead() { return g_dead; }
int sim_track_row_bytes() { return th::kRowBytes; }
int sim_track_rule_bytes() { return th::kRuleBytes; }
int sim_track_sort_tile() { return adsb_shared_host::kSortTile; }
unsigned long long sim_track_layout(long long n, unsigned long long* offs) {
  const th::Layout L = th::layout((size_t)n);
  const size_t at[14] = {L.cnts, L.stats, L.w, L.cnt, L.sel, L.run_start, L.run_len, L.pos, L.newidx, L.keys, L.keys_tmp, L.vals, L.vals_tmp, L.hist};
  if (offs) for (int k = 0; k < 14; ++k) offs[k] = at[k];
  return (unsigned long long)L.bytes;
}
unsigned sim_track_cover(long long work, int per) { return th::cover(work, per); }

int sim_track_update(const void* fixes, const void* aux, int ng, const void* rule, const void* store, int nt, void* store_out, int* nt_out,
                     long long* stats) {
  if (g_dead) return g_dead;
  return track_rule::update<Part>(group_end, fixes, aux, ng, rule, store, nt, store_out, nt_out, stats);
}
int sim_track_read(const void* store, int nt, int min_fixes, double cutoff, void* rows, int cap, int* n) {
  if (g_dead) return g_dead;
  return track_rule::read<Part>(group_end, store, nt, min_fixes, cutoff, false, rows, cap, n);
}
int sim_track_expire(const void* store, int nt, double cutoff, void* store_out, int* nt_out) {
  if (g_dead) return g_dead;
  return track_rule::read<Part>(group_end, store, nt, 0, cutoff, true, store_out, 0, nt_out);
}
}
