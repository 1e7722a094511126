// softfec_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's k_soft_fec / k_soft_fec_slices
// (gr_adsb_amd/csrc/adsb_softfec_device.h, the opt-in soft-decision CRC repair) on the SIMT emulator in hipsim.h, on host memory.
// Never linked into libadsb_hip.so.
#include "hipsim.h"

#include "../../gr_adsb_amd/csrc/adsb_softfec_device.h"

using namespace adsb_softfec;

namespace {
template <int MODE>
void run(const void* data, long long n, long long origin, float scale, int sps, const Rule& R, unsigned long long* recs, const int* n_kept,
         int out_cap, unsigned long long* mirror, int mirror_cap, unsigned long long* rows, int grid) {
  hipsim::launch(k_soft_fec<MODE>, (unsigned)grid, (unsigned)kThreads, data, n, origin, scale, sps, R, recs, n_kept, out_cap, mirror,
                 mirror ? mirror_cap : 0, rows);
}
}  // namespace

extern "C" {

// recs: out_cap records of 4 words, the first n_kept delivered; repaired in place by `grid` workgroups; mirror (may be null): a
// copy of the first mirror_cap records, repaired alongside; rows[out_cap]; mode: ADSB_FMT_*, data: n samples of that format
int sim_soft_records(int mode, const void* data, long long n, long long origin, float scale, int sps, const Rule* rule,
                     unsigned long long* recs, int n_kept, int out_cap, unsigned long long* mirror, int mirror_cap, unsigned long long* rows,
                     int grid) {
  switch (mode) {
    case 0: run<0>(data, n, origin, scale, sps, *rule, recs, &n_kept, out_cap, mirror, mirror_cap, rows, grid); break;
    case 1: run<1>(data, n, origin, scale, sps, *rule, recs, &n_kept, out_cap, mirror, mirror_cap, rows, grid); break;
    case 2: run<2>(data, n, origin, scale, sps, *rule, recs, &n_kept, out_cap, mirror, mirror_cap, rows, grid); break;
    case 3: run<3>(data, n, origin, scale, sps, *rule, recs, &n_kept, out_cap, mirror, mirror_cap, rows, grid); break;
    case 4: run<4>(data, n, origin, scale, sps, *rule, recs, &n_kept, out_cap, mirror, mirror_cap, rows, grid); break;
    default: return -1;
  }
  return 0;
}

int sim_soft_slices(const float* data, long long n, const long long* tag_idx, int sps, const Rule* rule, unsigned char* bits14,
                    unsigned char* ok, int ntags, unsigned long long* rows, int grid) {
  hipsim::launch(k_soft_fec_slices, (unsigned)grid, (unsigned)kThreads, (const void*)data, n, tag_idx, sps, *rule, bits14, ok, ntags, rows);
  return 0;
}
}
