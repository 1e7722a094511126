// dedup_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  The twin of tests/sim/dedup_driver.cpp's sim_dedup_step on the GPU: the
// same entry point with the same arguments, over the SHIPPED translation unit gr_adsb_amd/csrc/adsb_dedup.hip -- compiled as a
// unit of its own with the library's flags and linked beside this file into tests/gpu/libadsb_dedup_dev.so
// (tests/test_gpu_dedup_device.py builds it) -- and its real launchers launch_entries / launch_find / launch_merge /
// launch_mark with their own cover().  This file launches no k_dedup_* kernel itself and includes no device code.
//
// `grid` is accepted and IGNORED: the real launchers choose the grid.
//
// Every array lives in device memory as a part of its own (device_buffers.h): filled with the guard byte first, a guard tail
// behind it.  After each launcher all parts come back whole: a changed guard byte, or a changed byte of an input the kernels
// only read (the carry, order[], first[], item_stream[], sorted_ts[]; the records until k_dedup_find, the entries behind
// k_dedup_entries, dup[] behind k_dedup_find), is -1.  Every HIP call's status is checked: an error is -1000 - hipError_t, no
// further GPU call is made, and every later call of this library returns the same code at once (dev_dedup_dead).
// Never linked into libadsb_hip.so.
#include "device_buffers.h"

#include "../../gr_adsb_amd/csrc/adsb_dedup.h"

namespace dh = adsb_dedup_host;

static_assert(dh::kRecBytes == 32 && dh::kRowBytes == 72 && dh::kEntBytes == 32 && sizeof(dh::State) == 16, "the sizes adsb_dedup.h states");

extern "C" {

int dev_dedup_dead() { return g_dead; }

// sim_dedup_step (tests/sim/dedup_driver.cpp), argument for argument.  0; -1: a guard byte or a read-only input was
// overwritten; -5: a bad argument; -6: the cut k_dedup_merge states does not add up; <= -1000: a HIP status.
int sim_dedup_step(const unsigned long long* sorted_recs, const double* sorted_ts, const int* order, int n, const int* first,
                   const int* item_stream, int n_items, const unsigned long long* carry_in, int nc, double window, double horizon, int grid,
                   const unsigned long long* recs_in, const unsigned long long* rows_in, unsigned long long* ent_out, int* dup_out,
                   unsigned long long* sorted_out, unsigned long long* merged_out, void* state_out, unsigned long long* recs_out,
                   unsigned long long* rows_out) {
  (void)grid;
  if (n < 0 || nc < 0) return -5;
  if (n == 0) return 0;
  if (n_items <= 0 || first[0] != 0 || first[n_items] != n || !(window >= 0) || !(horizon >= 0)) return -5;
  for (int i = 0; i < n_items; ++i)
    if (first[i] > first[i + 1]) return -5;
  {
    std::vector<char> hit((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
      const int t = order[k];
      if (t < 0 || t >= n || hit[(size_t)t]) return -5;
      hit[(size_t)t] = 1;
    }
  }
  if (g_dead) return g_dead;
  const size_t nn = (size_t)n, rec = dh::kRecBytes, ent_b = dh::kEntBytes, row = dh::kRowBytes;
  Part srecs, sts, ord, fst, streams, carry, ent, dup, merged, state, recs, rows;
  if (srecs.make(sorted_recs, nn * rec, true) || sts.make(sorted_ts, nn * 8, true) || ord.make(order, nn * 4, true) ||
      fst.make(first, ((size_t)n_items + 1) * 4, true) || streams.make(item_stream, (size_t)n_items * 4, true) ||
      carry.make(nc ? carry_in : nullptr, (size_t)nc * ent_b, true) || ent.make(nullptr, nn * ent_b, false) || dup.make(nullptr, nn * 4, false) ||
      merged.make(nullptr, ((size_t)nc + nn) * ent_b, false) || state.make(nullptr, sizeof(dh::State), false) ||
      recs.make(recs_in, nn * rec, false) || rows.make(rows_in, nn * row, false))
    return g_dead;
  const hipStream_t st = nullptr;
  const auto all = {&srecs, &sts, &ord, &fst, &streams, &carry, &ent, &dup, &merged, &state, &recs, &rows};
  int rc;

  if ((rc = group_end(dh::launch_entries(st, srecs.p, sts.as<double>(), ord.as<int>(), n, fst.as<int>(), streams.as<int>(), n_items, ent.p), all)))
    return rc;
  memcpy(ent_out, ent.host.data(), nn * ent_b);
  srecs.read_only = false;                            // k_dedup_find takes ADSB_BURST_DEMOD from the duplicates

  if ((rc = group_end(dh::launch_find(st, ent.p, n, carry.p, nc, window, ord.as<int>(), srecs.p, dup.as<int>()), all))) return rc;
  if (!ent.equals(ent_out)) return -1;
  memcpy(dup_out, dup.host.data(), nn * 4);
  memcpy(sorted_out, srecs.host.data(), nn * rec);

  if ((rc = group_end(dh::launch_merge(st, carry.p, nc, ent.p, n, horizon, merged.p, state.p), all))) return rc;
  if (!ent.equals(ent_out) || !dup.equals(dup_out) || !srecs.equals(sorted_out)) return -1;
  memcpy(merged_out, merged.host.data(), ((size_t)nc + nn) * ent_b);
  memcpy(state_out, state.host.data(), sizeof(dh::State));

  if ((rc = group_end(dh::launch_mark(st, dup.as<int>(), n, recs.p, rows.p), all))) return rc;
  if (!ent.equals(ent_out) || !dup.equals(dup_out) || !srecs.equals(sorted_out) || !merged.equals(merged_out) || !state.equals(state_out)) return -1;
  memcpy(recs_out, recs.host.data(), nn * rec);
  memcpy(rows_out, rows.host.data(), nn * row);
  const dh::State s = *state.got<dh::State>();
  if (s.off < 0 || s.cnt < 1 || s.off + s.cnt != nc + n) return -6;
  return 0;
}
}
