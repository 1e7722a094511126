// decode_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's decode step (gr_adsb_amd/csrc/adsb_device.h:
// k_dec_pdu_flags, k_fec_slices, the aircraft-table kernels, k_dec_classify, k_dec_sort_*, k_dec_fold; ADSB_FLAG_DECODE) on
// the SIMT emulator in hipsim.h, on host memory, in the order adsb_hip.hip's adsb_decode_pdus / launch_air / launch_dec
// queue them.  Never linked into libadsb_hip.so.
#include "hipsim.h"

#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_device.h"

using namespace adsb;

namespace {
constexpr unsigned long long kGuard = 0xA5A5A5A5A5A5A5A5ull;

// The group stage as launch_dec queues it: shifts 32, 36, ... 56, each a histogram, a scan and a scatter, ping-pong between
// keys and sorted, the result in sorted.  Both hold n keys and kSortTile guard slots behind them: -1 when a kernel wrote one.
int sort_keys(std::vector<unsigned long long>& keys, std::vector<unsigned long long>& sorted, int n) {
  const int nblk = (n + kSortTile - 1) / kSortTile;
  std::vector<unsigned> hist((size_t)nblk * 16 + 16, 0xA5A5A5A5u);
  unsigned long long* in = keys.data();
  unsigned long long* out = sorted.data();
  for (int shift = 32; shift < 60; shift += 4) {
    hipsim::launch(k_dec_sort_hist, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, n, shift, hist.data());
    hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, hist.data(), nblk * 16);
    hipsim::launch(k_dec_sort_scatter, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, out, n, shift,
                   (const unsigned*)hist.data());
    unsigned long long* x = in; in = out; out = x;
  }
  for (int k = 0; k < kSortTile; ++k)
    if (keys[(size_t)n + k] != kGuard || sorted[(size_t)n + k] != kGuard) return -1;
  for (int k = 0; k < 16; ++k)
    if (hist[(size_t)nblk * 16 + k] != 0xA5A5A5A5u) return -1;
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
  std::vector<unsigned long long> a((size_t)n + kSortTile, kGuard), b((size_t)n + kSortTile, kGuard);
  for (int i = 0; i < n; ++i) a[i] = keys[i];
  const int r = sort_keys(a, b, n);
  for (int i = 0; i < n; ++i) out[i] = b[i];
  return r;
}

// n PDUs (bits14: n x 14, ts: n timestamps) as one call: rows = n x 72 bytes.  table = 2^24 keys, st = an AirState,
// planes = 2^24 Plane entries (all zero at first); pass = the call's number; epoch = the entries' epoch.
// -1 as above, -2: a sorted key that names no record of the call; the fold is not run then.
int sim_dec_pdus(unsigned char* bits14, const double* ts, int n, int grid, unsigned long long* table, void* st, void* planes,
                 unsigned epoch, unsigned long long pass, int fec, int all, void* rows) {
  std::vector<unsigned char> ok((size_t)n);
  std::vector<unsigned long long> keys((size_t)n + kSortTile, kGuard), sorted((size_t)n + kSortTile, kGuard);
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
  if (sort_keys(keys, sorted, n)) return -1;
  for (int i = 0; i < n; ++i)                                    // the fold reads the records these name
    if (sorted[i] != kDecNoKey && (unsigned)sorted[i] >= (unsigned)n) return -2;
  hipsim::launch(k_dec_fold, (unsigned)grid, (unsigned)kThreads, d);
  return 0;
}
}
