// adsb_shared.hip -- the translation unit of ADSB_FLAG_STREAM_DECODE_SHARED's kernels (adsb_shared_device.h) and their
// launchers (adsb_shared.h).  A unit of its own, so that the kernels of adsb_hip.hip are compiled exactly as they are without
// it; both are linked into libadsb_hip.so.
#include <hip/hip_runtime.h>

#include "adsb_shared.h"
#include "adsb_shared_device.h"

namespace adsb_shared_host {

using namespace adsb_shared;

static_assert(kRecBytes == kRecWords * 8 && kRowBytes == kRowWords * 8, "the header's sizes are the device code's");
static_assert(kSortTile == adsb_shared::kSortTile, "the header's tile is the device code's");

namespace {
// grid-stride kernels: enough workgroups to cover `work` threads, a few per compute unit at the most
unsigned cover(long long work) {
  const long long g = (work + kThreads - 1) / kThreads;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
int blocks(int n) { return (n + adsb_shared::kSortTile - 1) / adsb_shared::kSortTile; }
}  // namespace

size_t sort_hist_bytes(int n) { return (size_t)blocks(n) * kDigits * sizeof(unsigned); }

int launch_keys(void* stream, const void* recs, int n, const int* first, const double* start, int n_items, double fs,
                unsigned long long* keys, unsigned* vals, double* ts) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_shared_keys, dim3(cover(n)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)recs, n, first,
                     start, n_items, fs, keys, vals, ts);
  return (int)hipGetLastError();
}

int launch_sort(void* stream, unsigned long long* keys, unsigned* vals, unsigned long long* keys_tmp, unsigned* vals_tmp, int n,
                unsigned* hist) {
  if (n <= 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int nblk = blocks(n);
  unsigned long long *ki = keys, *ko = keys_tmp;
  unsigned *vi = vals, *vo = vals_tmp;
  for (int shift = 0; shift < 64; shift += kDigitBits) {
    hipLaunchKernelGGL(k_shared_sort_hist, dim3(nblk), dim3(kThreads), 0, st, (const unsigned long long*)ki, n, shift, hist);
    hipLaunchKernelGGL(k_shared_sort_scan, dim3(1), dim3(kThreads), 0, st, hist, nblk * kDigits);
    hipLaunchKernelGGL(k_shared_sort_scatter, dim3(nblk), dim3(kThreads), 0, st, (const unsigned long long*)ki, (const unsigned*)vi, ko, vo,
                       n, shift, (const unsigned*)hist);
    unsigned long long* k = ki; ki = ko; ko = k;
    unsigned* v = vi; vi = vo; vo = v;
  }
  return (int)hipGetLastError();
}

int launch_gather(void* stream, const void* recs, const double* ts, const unsigned* vals, int n, void* sorted_recs, double* sorted_ts,
                  int* order) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_shared_gather, dim3(cover(n)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)recs, ts, vals, n,
                     (unsigned long long*)sorted_recs, sorted_ts, order);
  return (int)hipGetLastError();
}

int launch_scatter(void* stream, const void* sorted_recs, const void* sorted_rows, const int* order, int n, void* recs, void* rows) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_shared_scatter, dim3(cover((long long)n * kRowWords)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const unsigned long long*)sorted_recs, (const unsigned long long*)sorted_rows, order, n, (unsigned long long*)recs,
                     (unsigned long long*)rows);
  return (int)hipGetLastError();
}

}  // namespace adsb_shared_host
