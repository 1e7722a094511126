// softfec_batch_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's k_soft_fec_batch
// (gr_adsb_amd/csrc/adsb_softfec_batch_device.h, the soft-decision CRC repair of a batch pass's packed list) on the SIMT emulator in
// hipsim.h, on host memory.  Never linked into libadsb_hip.so.
#include "hipsim.h"

#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_softfec_batch_device.h"

using namespace adsb_softfec_batch;

namespace {
template <int MODE>
void run(int n_items, const Item* items, const int* first, float scale, int sps, const Rule& R, unsigned long long* recs, int out_cap,
         unsigned long long* mirror, int mirror_cap, unsigned long long* rows) {
  hipsim::launch(k_soft_fec_batch<MODE>, (unsigned)n_items, (unsigned)kThreads, items, first, scale, sps, R, recs, out_cap, mirror,
                 mirror ? mirror_cap : 0, rows);
}
}  // namespace

extern "C" {

// Item i: data[i] = n[i] samples of format `mode`, sample 0 at stream offset origin[i]; its records are recs[first[i] ..
// first[i + 1]) of the packed list of out_cap records of 4 words, repaired in place by n_items workgroups (the grid is the
// items: the shipped launcher's); mirror (may be null): a copy of the first mirror_cap records, repaired alongside; rows[out_cap]
int sim_soft_batch(int mode, int n_items, const void* const* data, const long long* n, const long long* origin, const int* first,
                   float scale, int sps, const Rule* rule, unsigned long long* recs, int out_cap, unsigned long long* mirror, int mirror_cap,
                   unsigned long long* rows) {
  if (n_items <= 0 || out_cap <= 0) return 0;                      // (as the launcher)
  std::vector<Item> items((size_t)n_items);
  for (int i = 0; i < n_items; ++i) items[(size_t)i] = Item{data[i], n[i], origin[i], 0};
  switch (mode) {
    case 0: run<0>(n_items, items.data(), first, scale, sps, *rule, recs, out_cap, mirror, mirror_cap, rows); break;
    case 1: run<1>(n_items, items.data(), first, scale, sps, *rule, recs, out_cap, mirror, mirror_cap, rows); break;
    case 2: run<2>(n_items, items.data(), first, scale, sps, *rule, recs, out_cap, mirror, mirror_cap, rows); break;
    case 3: run<3>(n_items, items.data(), first, scale, sps, *rule, recs, out_cap, mirror, mirror_cap, rows); break;
    case 4: run<4>(n_items, items.data(), first, scale, sps, *rule, recs, out_cap, mirror, mirror_cap, rows); break;
    default: return -1;
  }
  return 0;
}
}
