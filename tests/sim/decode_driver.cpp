// decode_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's decode step (gr_adsb_amd/csrc/adsb_device.h:
// k_dec_pdu_flags, k_fec_slices, the aircraft-table kernels, k_dec_classify, k_dec_sort_*, k_dec_fold or, with a last_seen
// array, k_ages_fold; ADSB_FLAG_DECODE) on the SIMT emulator in hipsim.h, on host memory, in the order adsb_hip.hip's
// adsb_decode_pdus / launch_air / launch_dec queue them.  Never linked into libadsb_hip.so.
#include "sim_support.h"

using namespace adsb;

namespace {
// n PDUs as one call; seen: the last_seen array (2^24 int64, never cleared: any bytes at first), or null
int dec_pdus(unsigned char* bits14, const double* ts, int n, int grid, unsigned long long* table, void* st, void* planes, long long* seen,
             unsigned epoch, unsigned long long pass, int fec, int all, void* rows) {
  std::vector<unsigned char> ok((size_t)n);
  KeyPair k((size_t)n);
  hipsim::launch(k_dec_pdu_flags, (unsigned)grid, (unsigned)kThreads, (const unsigned char*)bits14, ok.data(), n);
  if (fec) hipsim::launch(k_fec_slices, (unsigned)grid, (unsigned)kThreads, bits14, ok.data(), n);
  AirArgs a{};
  a.bits14 = bits14; a.ok = ok.data(); a.cap = n; a.table = table; a.st = (AirState*)st; a.pass = pass << 32; a.fec = fec;
  hipsim::launch(k_air_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_air_cond, 1u, 64u, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  DecArgs d{};
  d.air = a; d.ts = ts; d.planes = (Plane*)planes; d.epoch = epoch; d.all = all; d.keys = k.keys.p(); d.sorted = k.sorted.p();
  d.rows = (DecRow*)rows; d.seen = seen;
  hipsim::launch(k_dec_classify, (unsigned)grid, (unsigned)kThreads, d);
  if (sort_keys(k.keys.p(), k.sorted.p(), n, 32, 60) || !k.ok()) return -1;
  for (int i = 0; i < n; ++i)                                    // the fold reads the records these name
    if (k.sorted.p()[i] != kDecNoKey && (unsigned)k.sorted.p()[i] >= (unsigned)n) return -2;
  if (seen) hipsim::launch(k_ages_fold, (unsigned)grid, (unsigned)kThreads, d);         // launch_dec's choice
  else hipsim::launch(k_dec_fold, (unsigned)grid, (unsigned)kThreads, d);
  return 0;
}
}  // namespace

extern "C" {

int sim_air_state_bytes() { return (int)sizeof(AirState); }
int sim_dec_plane_bytes() { return (int)sizeof(Plane); }
int sim_dec_row_bytes() { return (int)sizeof(DecRow); }
int sim_dec_sort_tile() { return kSortTile; }

// The sort alone: n keys -> out (n keys), by bits 32..59, stable.  -1: a kernel wrote outside its n keys.
int sim_dec_sort(const unsigned long long* keys, int n, unsigned long long* out) {
  if (n <= 0) return 0;
  KeyPair k((size_t)n);
  memcpy(k.keys.p(), keys, (size_t)n * 8);
  const int r = sort_keys(k.keys.p(), k.sorted.p(), n, 32, 60);
  memcpy(out, k.sorted.p(), (size_t)n * 8);
  return r || !k.ok() ? -1 : 0;
}

// n PDUs (bits14: n x 14, ts: n timestamps) as one call: rows = n x 72 bytes.  table = 2^24 keys, st = an AirState,
// planes = 2^24 Plane entries (all zero at first); pass = the call's number; epoch = the entries' epoch.
// -1 as above, -2: a sorted key that names no record of the call; the fold is not run then.
int sim_dec_pdus(unsigned char* bits14, const double* ts, int n, int grid, unsigned long long* table, void* st, void* planes,
                 unsigned epoch, unsigned long long pass, int fec, int all, void* rows) {
  return dec_pdus(bits14, ts, n, grid, table, st, planes, nullptr, epoch, pass, fec, all, rows);
}
}
