// adsb_dedup.hip -- the translation unit of ADSB_FLAG_STREAM_DEDUP's kernels (adsb_dedup_device.h) and their launchers
// (adsb_dedup.h).  A unit of its own, so that the kernels of adsb_hip.hip and adsb_shared.hip are compiled exactly as they are
// without it; all three are linked into libadsb_hip.so.
#include <hip/hip_runtime.h>

#include "adsb_dedup.h"
#include "adsb_dedup_device.h"

namespace adsb_dedup_host {

using namespace adsb_dedup;

static_assert(kRecBytes == kRecWords * 8 && kRowBytes == kRowWords * 8 && kEntBytes == kEntWords * 8, "the header's sizes are the device code's");
static_assert(sizeof(State) == sizeof(adsb_dedup::State) && sizeof(State) == 16, "the header's State is the device code's");

namespace {
// grid-stride kernels: enough workgroups to cover `work` threads, a few per compute unit at the most
unsigned cover(long long work) {
  const long long g = (work + kThreads - 1) / kThreads;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
}  // namespace

int launch_entries(void* stream, const void* sorted_recs, const double* sorted_ts, const int* order, int n, const int* first,
                   const int* item_stream, int n_items, void* ent) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_dedup_entries, dim3(cover(n)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)sorted_recs,
                     sorted_ts, order, n, first, item_stream, n_items, (unsigned long long*)ent);
  return (int)hipGetLastError();
}

int launch_find(void* stream, const void* ent, int n, const void* carry, int nc, double window, const int* order, void* sorted_recs,
                int* dup) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_dedup_find, dim3(cover(n)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)ent, n,
                     (const unsigned long long*)carry, nc, window, order, (unsigned long long*)sorted_recs, dup);
  return (int)hipGetLastError();
}

int launch_merge(void* stream, const void* carry, int nc, const void* ent, int n, double horizon, void* out, void* state) {
  if (nc + n <= 0) return 0;
  hipLaunchKernelGGL(k_dedup_merge, dim3(cover((long long)nc + n)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const unsigned long long*)carry, nc, (const unsigned long long*)ent, n, horizon, (unsigned long long*)out,
                     (adsb_dedup::State*)state);
  return (int)hipGetLastError();
}

int launch_mark(void* stream, const int* dup, int n, void* recs, void* rows) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_dedup_mark, dim3(cover(n)), dim3(kThreads), 0, (hipStream_t)stream, dup, n, (unsigned long long*)recs,
                     (unsigned long long*)rows);
  return (int)hipGetLastError();
}

}  // namespace adsb_dedup_host
