// adsb_mlat.hip -- the translation unit of adsb_stream_mlat's kernels (adsb_mlat_device.h) and their launchers (adsb_mlat.h).
// A unit of its own, so that the kernels of adsb_hip.hip, adsb_shared.hip and adsb_dedup.hip are compiled exactly as they are
// without it; all four are linked into libadsb_hip.so.
#include <hip/hip_runtime.h>

#include "adsb_mlat.h"
#include "adsb_mlat_device.h"

namespace adsb_mlat_host {

using namespace adsb_mlat;

static_assert(kEntBytes == kEntWords * 8 && kFixBytes == sizeof(Fix) && kChunk == kThreads && kMinRx == 4, "the header's sizes are the device code's");

namespace {
// w[n] (n = span[1] - span[0] <= n_max) -> idx / first of the values >= min_w; tot = {0, count, sum, 0}
void compact(hipStream_t st, const int* w, const int* span, int n_max, int min_w, int* cnt, int* sum, int* tot, int add_lo, int* idx, int* first) {
  const unsigned g = cover(n_max, kThreads);
  hipLaunchKernelGGL(k_mlat_count, dim3(g), dim3(kThreads), 0, st, w, span, min_w, cnt, sum);
  hipLaunchKernelGGL(k_mlat_scan, dim3(1), dim3(kThreads), 0, st, span, cnt, sum, tot);
  hipLaunchKernelGGL(k_mlat_place, dim3(g), dim3(kThreads), 0, st, w, span, min_w, (const int*)cnt, (const int*)sum, add_lo, idx, first);
}
}  // namespace

int launch_heads(void* stream, const void* carry, int nc, double t_lo, double t_hi, double window, void* work, const Layout& L) {
  if (nc <= 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned long long* c = (const unsigned long long*)carry;
  int* const range = part<int>(work, L.range);
  hipLaunchKernelGGL(k_mlat_range, dim3(1), dim3(kWave), 0, st, c, nc, t_lo, t_hi, range);
  hipLaunchKernelGGL(k_mlat_heads, dim3(cover(nc, kThreads)), dim3(kThreads), 0, st, c, nc, (const int*)range, window, part<int>(work, L.w));
  compact(st, part<int>(work, L.w), range, nc, 1, part<int>(work, L.cnt), part<int>(work, L.sum), part<int>(work, L.tot_heads), 1,
          part<int>(work, L.heads), nullptr);
  return (int)hipGetLastError();
}

int launch_groups(void* stream, const void* carry, int nc, int nh, double window, int min_rx, int n_streams, void* work, const Layout& L) {
  if (nh <= 0) return 0;
  hipLaunchKernelGGL(k_mlat_groups, dim3(cover(nh, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)carry, nc,
                     (const int*)part<int>(work, L.heads), (const int*)part<int>(work, L.tot_heads), window,
                     (const double*)part<double>(work, L.rx), n_streams, part<int>(work, L.nrx));
  const int e = (int)hipGetLastError();
  return e ? e : launch_select(stream, nh, min_rx, work, L);
}

int launch_select(void* stream, int nh, int min_rx, void* work, const Layout& L) {
  if (nh <= 0) return 0;
  compact((hipStream_t)stream, part<int>(work, L.nrx), part<int>(work, L.tot_heads), nh, min_rx, part<int>(work, L.cnt), part<int>(work, L.sum),
          part<int>(work, L.tot_groups), 0, part<int>(work, L.gsel), part<int>(work, L.gfirst));
  return (int)hipGetLastError();
}

int launch_solve(void* stream, const void* carry, int nc, int ng, double window, int n_streams, void* work, const Layout& L) {
  if (ng <= 0) return 0;
  hipLaunchKernelGGL(k_mlat_solve, dim3(cover(ng, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)carry, nc,
                     (const int*)part<int>(work, L.heads), (const int*)part<int>(work, L.gsel), (const int*)part<int>(work, L.gfirst),
                     (const int*)part<int>(work, L.tot_groups), window, (const double*)part<double>(work, L.rx), n_streams,
                     part<Fix>(work, L.fixes), part<int>(work, L.member_stream), part<double>(work, L.member_ts));
  return (int)hipGetLastError();
}

}  // namespace adsb_mlat_host
