// decode_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's decode step (gr_adsb_amd/csrc/adsb_device.h:
// k_dec_pdu_flags, k_fec_slices, the aircraft-table kernels, k_dec_classify, k_dec_fold; ADSB_FLAG_DECODE) on the SIMT
// emulator in hipsim.h, on host memory, in the order adsb_hip.hip's adsb_decode_pdus / launch_air queue them.  The group
// stage (a stable sort of the keys by address) runs on the host.  Never linked into libadsb_hip.so.
#include "hipsim.h"

#include <algorithm>
#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_device.h"

using namespace adsb;

extern "C" {

int sim_air_state_bytes() { return (int)sizeof(AirState); }
int sim_dec_plane_bytes() { return (int)sizeof(Plane); }
int sim_dec_row_bytes() { return (int)sizeof(DecRow); }

// n PDUs (bits14: n x 14, ts: n timestamps) as one call: rows = n x 72 bytes.  table = 2^24 keys, st = an AirState,
// planes = 2^24 Plane entries (all zero at first); pass = the call's number; epoch = the entries' epoch.
int sim_dec_pdus(unsigned char* bits14, const double* ts, int n, int grid, unsigned long long* table, void* st, void* planes,
                 unsigned epoch, unsigned long long pass, int fec, int all, void* rows) {
  std::vector<unsigned char> ok((size_t)n);
  std::vector<unsigned long long> keys((size_t)n), sorted((size_t)n);
  hipsim::launch(k_dec_pdu_flags, (unsigned)grid, (unsigned)kThreads, (const unsigned char*)bits14, ok.data(), n);
  if (fec) hipsim::launch(k_fec_slices, (unsigned)grid, (unsigned)kThreads, bits14, ok.data(), n);
  AirArgs a{};
  a.bits14 = bits14; a.ok = ok.data(); a.cap = n; a.table = table; a.st = (AirState*)st; a.pass = pass << 32; a.fec = fec;
  hipsim::launch(k_air_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_air_cond, 1u, 64u, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  DecArgs d{};
  d.air = a; d.ts = ts; d.planes = (Plane*)planes; d.epoch = epoch; d.all = all; d.keys = keys.data(); d.sorted = sorted.data();
  d.rows = (DecRow*)rows;
  hipsim::launch(k_dec_classify, (unsigned)grid, (unsigned)kThreads, d);
  sorted = keys;
  std::stable_sort(sorted.begin(), sorted.end(), [](unsigned long long x, unsigned long long y) {
    return ((x >> 32) & 0xFFFFFFFu) < ((y >> 32) & 0xFFFFFFFu);
  });
  hipsim::launch(k_dec_fold, (unsigned)grid, (unsigned)kThreads, d);
  return 0;
}
}
