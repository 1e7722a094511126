// softfec_batch_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  Runs k_soft_fec_batch ON THE DEVICE through the shipped launcher
// of gr_adsb_amd/csrc/adsb_softfec_batch.hip (compiled beside this file as the library compiles it: tests/device_build.py),
// every buffer -- each item's samples apart -- in device memory with a guard tail behind it (device_buffers.h).  The entry
// point has the signature of the emulator driver tests/sim/softfec_batch_driver.cpp, so that
// tests/test_gpu_softfec_batch_device.py runs the cases of tests/test_softfec_batch.py unchanged.
// -> 0, -1 (a guard byte or a read-only part changed) or -1000 - hipError_t (sticky).
#include "device_buffers.h"

#include <memory>

#include "../../gr_adsb_amd/csrc/adsb_softfec_batch.h"

extern "C" {

int sim_soft_batch(int mode, int n_items, const void* const* data, const long long* n, const long long* origin, const int* first,
                   float scale, int sps, const void* rule, unsigned long long* recs, int out_cap, unsigned long long* mirror, int mirror_cap,
                   unsigned long long* rows) {
  if (g_dead) return g_dead;
  if (n_items <= 0 || out_cap <= 0) return 0;
  using adsb_softfec_batch_host::Item;
  const size_t sample = mode == 0 ? 8 : mode <= 2 ? 4 : 2, rec = adsb_softfec_batch_host::kRecWords * 8, row = adsb_softfec_batch_host::kRowBytes;
  if (!mirror) mirror_cap = 0;
  std::vector<std::unique_ptr<Part>> d_data;
  std::vector<Item> items((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    d_data.emplace_back(new Part());
    if (d_data.back()->make(data[i], (size_t)n[i] * sample, true)) return g_dead;
    items[(size_t)i] = Item{d_data.back()->p, n[i], origin[i], 0};
  }
  Part d_items, d_first, d_recs, d_mirror, d_rows;
  if (d_items.make(items.data(), (size_t)n_items * sizeof(Item), true) || d_first.make(first, ((size_t)n_items + 1) * sizeof(int), true) ||
      d_recs.make(recs, (size_t)out_cap * rec, false) || d_mirror.make(mirror, (size_t)mirror_cap * rec, false) ||
      d_rows.make(rows, (size_t)out_cap * row, false))
    return g_dead;
  const int e = adsb_softfec_batch_host::launch_items(nullptr, n_items, mode, d_items.p, d_first.as<int>(), scale, sps, rule, d_recs.p, out_cap,
                                                      mirror ? d_mirror.p : nullptr, mirror_cap, d_rows.p);
  int rc = group_end(e, {&d_items, &d_first, &d_recs, &d_mirror, &d_rows});
  if (g_dead) return g_dead;
  for (auto& q : d_data) {
    const int r = q->back();
    if (g_dead) return g_dead;
    if (r) rc = r;
  }
  if (rc) return rc;
  memcpy(recs, d_recs.host.data(), (size_t)out_cap * rec);
  if (mirror_cap) memcpy(mirror, d_mirror.host.data(), (size_t)mirror_cap * rec);
  memcpy(rows, d_rows.host.data(), (size_t)out_cap * row);
  return 0;
}
}
