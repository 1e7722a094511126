// sim_support.h -- TEST INFRASTRUCTURE ONLY.  What the decoder drivers beside it share: guarded arrays, the host's refusal
// codes and the library's key sort (gr_adsb_amd/csrc/adsb_device.h: k_dec_sort_*) in the order adsb_hip.hip's launch_key_sort
// queues it.  A driver that counts the store's claims defines ADSB_FLEET_CAS before it includes this (fleet_driver.cpp).
// Never linked into libadsb_hip.so.
#pragma once
#include "hipsim.h"

#include <algorithm>
#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_device.h"

namespace {
constexpr unsigned char kGuardByte = 0xA5;
constexpr size_t kGuardBytes = 256;
constexpr int kNoSpace = -28, kInvalid = -22;

// n elements a kernel may touch and guard bytes behind them
template <class T>
struct Guarded {
  std::vector<unsigned char> raw;
  size_t n = 0, tail = kGuardBytes;
  Guarded() = default;
  Guarded(size_t n_, int fill, size_t tail_ = kGuardBytes) { reset(n_, fill, tail_); }
  void reset(size_t n_, int fill, size_t tail_ = kGuardBytes) {
    n = n_; tail = tail_;
    raw.assign(n * sizeof(T) + tail, kGuardByte);
    std::fill(raw.begin(), raw.begin() + (long)(n * sizeof(T)), (unsigned char)fill);
  }
  T* p() { return reinterpret_cast<T*>(raw.data()); }
  bool ok() const {
    for (size_t k = n * sizeof(T); k < raw.size(); ++k) if (raw[k] != kGuardByte) return false;
    return true;
  }
};

// keys and their ping-pong partner: n keys each and a sort tile of guard bytes behind them (what a scatter may not touch)
struct KeyPair {
  Guarded<unsigned long long> keys, sorted;
  explicit KeyPair(size_t n) : keys(n, 0xA5, (size_t)kSortTile * 8), sorted(n, 0xA5, (size_t)kSortTile * 8) {}
  bool ok() const { return keys.ok() && sorted.ok(); }
};

// The stable sort of in[0 .. n) by the bits [lo_bit, hi_bit), a nibble a pass: a histogram, a scan and a scatter, ping-pong
// between in and out.  Both ranges in use (32..60: the decode step; 0..44: the store's keys) give an odd number of passes:
// the result is in out.  0, or -1: a kernel wrote behind the histogram (the callers guard the keys)
inline int sort_keys(unsigned long long* in, unsigned long long* out, int n, int lo_bit, int hi_bit) {
  assert(((hi_bit - lo_bit + 3) / 4) % 2 == 1);
  const int nblk = (n + kSortTile - 1) / kSortTile;
  Guarded<unsigned> hist((size_t)nblk * 16, 0xA5);
  for (int shift = lo_bit; shift < hi_bit; shift += 4) {
    hipsim::launch(k_dec_sort_hist, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, n, shift, hist.p());
    hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, hist.p(), nblk * 16);
    hipsim::launch(k_dec_sort_scatter, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, out, n, shift,
                   (const unsigned*)hist.p());
    std::swap(in, out);
  }
  return hist.ok() ? 0 : -1;
}
}  // namespace
