// adsb_shared_device.h -- device code of ADSB_FLAG_STREAM_DECODE_SHARED: the time order of one stream-batch call.
//
// A shared context puts ONE decoder behind all of its receiver streams (the reference's fan-in of several demod blocks into
// one decoder block, decoder.py:325-352: one plane_dict, fed in arrival order).  The decode step itself is the per-stream
// one (adsb_device.h: k_fleet_*), run unchanged on a list with one item; what this header adds is the order that list is
// in -- ascending (PDU timestamp, position in the call's list) -- and the way back:
//
//   k_shared_keys     per record: its item by binary search over first[], ts = start[item] + (double)offset / fs (the
//                     expression of k_fleet_classify, bit for bit), key = a monotone map of the double's bits, val = position
//   k_shared_sort_*   a stable LSD radix sort of (64-bit key, 32-bit position) pairs: eight passes of eight bits, each a
//                     block histogram, one scan, a stable scatter.  Stability and input in list order give the tie rule.
//                     Deterministic: an output position is offset[digit] + ranks counted by ballots, never an atomic's
//                     return value (the histogram's LDS atomics only count).
//   k_shared_gather   sorted_recs[r] = recs[order[r]], sorted_ts[r] = ts[order[r]], order[] itself
//   k_shared_scatter  after the decode step: record word 3 (the verdict flags) and the rows back to list positions
//
// Records (32 bytes) and rows (72 bytes) are moved as opaque 64-bit words; a record's offset is its word 0, its flags are
// in word 3.  adsb_hip.hip ties both sizes to Rec and DecRow.
//
// This header contains device code only, includes nothing and does not need adsb_device.h.  The includer provides the HIP
// device environment (adsb_shared.hip), or the SIMT emulator of tests/sim/hipsim.h.
#pragma once

namespace adsb_shared {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRecWords = 4, kRowWords = 9;          // 32-byte records, 72-byte rows
constexpr int kDigitBits = 8, kDigits = 1 << kDigitBits, kPasses = 64 / kDigitBits;
// 4096 pairs per workgroup as in the decode step's key sort: sixteen rounds of one pair per thread.  5 KiB of LDS in the
// scatter (the running offsets and one count per wavefront and digit), 1 KiB in the histogram.
constexpr int kSortItems = 16, kSortTile = kThreads * kSortItems;
static_assert(kDigits == kThreads, "one thread per digit in the histogram's write-out and the scatter's offsets");
static_assert(kPasses % 2 == 0, "an even number of passes: the result ends in the buffers the keys were written to");

// Ascending keys <=> ascending doubles: a set sign bit flips every bit (more negative: smaller), a clear one sets it.
// -0.0 takes +0.0's key -- they compare equal, so list order decides between them.
__device__ __forceinline__ unsigned long long time_key(double ts) {
  unsigned long long b = (unsigned long long)__double_as_longlong(ts);
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// first[0 .. n_items]: the items' first records, first[n_items] = n (empty items share their successor's); start[n_items]
__global__ void __launch_bounds__(kThreads) k_shared_keys(const unsigned long long* recs, int n, const int* first, const double* start,
                                                          int n_items, double fs, unsigned long long* keys, unsigned* vals, double* ts) {
  for (int t = (int)(blockIdx.x * kThreads + threadIdx.x); t < n; t += (int)(gridDim.x * kThreads)) {
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {                                 // the last item whose first record is not behind t
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const double v = start[lo] + (double)(long long)recs[(long long)t * kRecWords] / fs;
    ts[t] = v;
    keys[t] = time_key(v);
    vals[t] = (unsigned)t;
  }
}

// hist[digit * gridDim.x + block]: the block's pairs whose key has that digit at `shift`
__global__ void __launch_bounds__(kThreads) k_shared_sort_hist(const unsigned long long* keys, int n, int shift, unsigned* hist) {
  __shared__ unsigned cnt[kDigits];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int base = (int)blockIdx.x * kSortTile;
  for (int r = 0; r < kSortItems; ++r) {
    const int i = base + r * kThreads + (int)threadIdx.x;
    if (i < n) atomicAdd(&cnt[(unsigned)(keys[i] >> shift) & (unsigned)(kDigits - 1)], 1u);
  }
  __syncthreads();
  hist[threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of hist[total] (digit-major), one workgroup
__global__ void __launch_bounds__(kThreads) k_shared_sort_scan(unsigned* hist, int total) {
  __shared__ unsigned wsum[kWaves];
  __shared__ unsigned carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  for (int base = 0; base < total; base += kThreads) {
    const int i = base + (int)threadIdx.x;
    const unsigned v = i < total ? hist[i] : 0u;
    unsigned x = v;
    for (int o = 1; o < 64; o <<= 1) { const unsigned y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned pre = carry;
    for (int w = 0; w < wave; ++w) pre += wsum[w];
    if (i < total) hist[i] = pre + x - v;
    __syncthreads();
    if (threadIdx.x == kThreads - 1) carry = pre + x;
    __syncthreads();
  }
}

// One round moves 256 consecutive pairs: a pair's place is the block's running offset of its digit, plus the pairs with
// that digit in the wavefronts in front, plus those in the lanes in front -- the lanes that share a digit are found with
// one ballot per digit bit.
__global__ void __launch_bounds__(kThreads) k_shared_sort_scatter(const unsigned long long* keys_in, const unsigned* vals_in,
                                                                  unsigned long long* keys_out, unsigned* vals_out, int n, int shift,
                                                                  const unsigned* hist) {
  __shared__ unsigned off[kDigits];
  __shared__ unsigned wcnt[kWaves][kDigits];
  off[threadIdx.x] = hist[threadIdx.x * gridDim.x + blockIdx.x];
  for (int w = 0; w < kWaves; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int base = (int)blockIdx.x * kSortTile;
  for (int r = 0; r < kSortItems; ++r) {
    const int i = base + r * kThreads + (int)threadIdx.x;
    const bool live = i < n;
    const unsigned long long k = live ? keys_in[i] : 0ull;
    const unsigned v = live ? vals_in[i] : 0u;
    const unsigned d = (unsigned)(k >> shift) & (unsigned)(kDigits - 1);
    unsigned long long peers = __ballot(live);
    for (int b = 0; b < kDigitBits; ++b) {
      const unsigned long long m = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? m : ~m;
    }
    const unsigned rank = (unsigned)__popcll(peers & lt);
    if (live && rank == 0) wcnt[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    if (live) {
      unsigned pos = off[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      keys_out[pos] = k;
      vals_out[pos] = v;
    }
    __syncthreads();
    unsigned t = 0;
    for (int w = 0; w < kWaves; ++w) { t += wcnt[w][threadIdx.x]; wcnt[w][threadIdx.x] = 0; }
    off[threadIdx.x] += t;
    __syncthreads();
  }
}

// vals: the sorted positions.  One thread per place r of the time order.
__global__ void __launch_bounds__(kThreads) k_shared_gather(const unsigned long long* recs, const double* ts, const unsigned* vals, int n,
                                                            unsigned long long* sorted_recs, double* sorted_ts, int* order) {
  for (int r = (int)(blockIdx.x * kThreads + threadIdx.x); r < n; r += (int)(gridDim.x * kThreads)) {
    const unsigned t = vals[r];
    if (t >= (unsigned)n) continue;                   // (a permutation of 0 .. n-1: never)
    const unsigned long long* s = recs + (long long)t * kRecWords;
    unsigned long long* d = sorted_recs + (long long)r * kRecWords;
    for (int w = 0; w < kRecWords; ++w) d[w] = s[w];
    sorted_ts[r] = ts[t];
    order[r] = (int)t;
  }
}

// One thread per row word: word 0's thread also takes the record's verdict flags home.
__global__ void __launch_bounds__(kThreads) k_shared_scatter(const unsigned long long* sorted_recs, const unsigned long long* sorted_rows,
                                                             const int* order, int n, unsigned long long* recs, unsigned long long* rows) {
  const long long total = (long long)n * kRowWords;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int r = (int)(i / kRowWords), w = (int)(i % kRowWords);
    const unsigned t = (unsigned)order[r];
    if (t >= (unsigned)n) continue;
    rows[(long long)t * kRowWords + w] = sorted_rows[i];
    if (w == 0) recs[(long long)t * kRecWords + 3] = sorted_recs[(long long)r * kRecWords + 3];
  }
}

}  // namespace adsb_shared
