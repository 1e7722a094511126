// fec_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's k_fec / k_fec_slices (gr_adsb_amd/csrc/adsb_device.h, the
// opt-in Conservative error correction) on the SIMT emulator in hipsim.h, on host memory.  Never linked into libadsb_hip.so.
#include "hipsim.h"

#include "../../gr_adsb_amd/csrc/adsb_device.h"

using namespace adsb;

extern "C" {

// recs: n records of 4 words, repaired in place by `grid` workgroups; mirror (may be null): a copy of the first mirror_cap
// records, repaired alongside (the pinned host copy of a mid-size pass)
int sim_fec(unsigned long long* recs, int n, int grid, unsigned long long* mirror, int mirror_cap) {
  Summary sum{};
  sum.n_kept = n;
  hipsim::launch(k_fec, (unsigned)grid, (unsigned)kThreads, (Rec*)recs, (const Summary*)&sum, n, (Rec*)mirror, mirror ? mirror_cap : 0);
  return 0;
}

int sim_fec_slices(unsigned char* bits14, unsigned char* ok, int ntags, int grid) {
  hipsim::launch(k_fec_slices, (unsigned)grid, (unsigned)kThreads, bits14, ok, ntags);
  return 0;
}
}
