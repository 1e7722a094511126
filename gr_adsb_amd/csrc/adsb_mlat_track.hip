// adsb_mlat_track.hip -- the translation unit of the MLAT track store's kernels (adsb_mlat_track_device.h) and their launchers
// (adsb_mlat_track.h).  A sixth unit, so that the kernels of the other five and their resource reports are exactly what they are
// without it; it sorts with adsb_shared.hip's launch_sort and defines no sort of its own.  Linked into libadsb_hip.so.
#include <hip/hip_runtime.h>

#include <string.h>

#include "adsb_mlat_track.h"
#include "adsb_mlat_track_device.h"

namespace adsb_mlat_track_host {

using namespace adsb_mlat_track;

static_assert(kRowBytes == sizeof(Track) && kRowBytes == kRowWords * 8 && kRuleBytes == sizeof(Rule) && kFixBytes == sizeof(Fix) &&
              kAuxBytes == sizeof(Aux) && kChunk == kThreads, "the header's sizes are the device code's");
static_assert(kCntWords == adsb_mlat_track::kCntWords && kStatWords == adsb_mlat_track::kStatWords && kCntKeys == adsb_mlat_track::kCntKeys &&
              kCntRuns == adsb_mlat_track::kCntRuns && kCntNew == adsb_mlat_track::kCntNew && kStatUnusable == kUnusable && kStatStale == kStale &&
              kStatRejected == kRejected && kStatTaken == kTaken && kStatStarted == kStarted, "the header's words are the device code's");

namespace {
// w[*np] (*np <= n_max) -> idx[] = the indices of the set flags, *tot = their number
void compact(hipStream_t st, const int* w, const int* np, int n_max, int* cnt, int* tot, int* idx) {
  const unsigned g = cover(n_max, kThreads);
  hipLaunchKernelGGL(k_track_count, dim3(g), dim3(kThreads), 0, st, w, np, cnt);
  hipLaunchKernelGGL(k_track_scan, dim3(1), dim3(kThreads), 0, st, np, cnt, tot);
  hipLaunchKernelGGL(k_track_place, dim3(g), dim3(kThreads), 0, st, w, np, (const int*)cnt, idx);
}
}  // namespace

int launch_keys(void* stream, const void* fixes, int ng, void* work, const Layout& L) {
  if (ng <= 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  int* const cnts = part<int>(work, L.cnts);
  const unsigned g = cover(ng, kThreads);
  hipLaunchKernelGGL(k_track_eligible, dim3(g), dim3(kThreads), 0, st, (const Fix*)fixes, ng, part<int>(work, L.w), cnts,
                     part<unsigned long long>(work, L.stats));
  compact(st, part<int>(work, L.w), cnts + kCntIn, ng, part<int>(work, L.cnt), cnts + kCntKeys, part<int>(work, L.sel));
  hipLaunchKernelGGL(k_track_keys, dim3(g), dim3(kThreads), 0, st, (const Fix*)fixes, (const int*)part<int>(work, L.sel),
                     (const int*)(cnts + kCntKeys), part<unsigned long long>(work, L.keys), part<unsigned>(work, L.vals));
  return (int)hipGetLastError();
}

int launch_update(void* stream, const void* fixes, const void* aux, int nk, const void* rule, const void* store, int nt, void* next, void* work,
                  const Layout& L) {
  if (nk <= 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  Rule R;
  memcpy(&R, rule, sizeof R);
  int* const cnts = part<int>(work, L.cnts);
  unsigned long long* const keys = part<unsigned long long>(work, L.keys);
  int* const w = part<int>(work, L.w);
  int* const run_start = part<int>(work, L.run_start);
  int* const newidx = part<int>(work, L.newidx);
  const int e = adsb_shared_host::launch_sort(stream, keys, part<unsigned>(work, L.vals), part<unsigned long long>(work, L.keys_tmp),
                                              part<unsigned>(work, L.vals_tmp), nk, part<unsigned>(work, L.hist));
  if (e) return e;
  const unsigned g = cover(nk, kThreads);
  hipLaunchKernelGGL(k_track_heads, dim3(g), dim3(kThreads), 0, st, (const unsigned long long*)keys, (const int*)(cnts + kCntKeys), w);
  compact(st, w, cnts + kCntKeys, nk, part<int>(work, L.cnt), cnts + kCntRuns, run_start);
  hipLaunchKernelGGL(k_track_find, dim3(g), dim3(kThreads), 0, st, (const unsigned long long*)keys, (const int*)run_start,
                     (const int*)(cnts + kCntRuns), (const int*)(cnts + kCntKeys), (const Fix*)fixes, (const Aux*)aux, R, (const Track*)store, nt,
                     part<int>(work, L.run_len), part<int>(work, L.pos), w);
  compact(st, w, cnts + kCntRuns, nk, part<int>(work, L.cnt), cnts + kCntNew, newidx);
  if (nt > 0)
    hipLaunchKernelGGL(k_track_move, dim3(cover((long long)nt * kRowWords, kThreads)), dim3(kThreads), 0, st, (const Track*)store, nt,
                       (const unsigned long long*)keys, (const int*)run_start, (const int*)newidx, (const int*)(cnts + kCntNew), (Track*)next);
  hipLaunchKernelGGL(k_track_update, dim3(g), dim3(kThreads), 0, st, (const unsigned long long*)keys, (const int*)run_start,
                     (const int*)part<int>(work, L.run_len), (const int*)part<int>(work, L.pos), (const int*)(cnts + kCntRuns), (const int*)newidx,
                     (const int*)(cnts + kCntNew), (const Fix*)fixes, (const Aux*)aux, R, (const Track*)store, nt, (Track*)next,
                     part<unsigned long long>(work, L.stats));
  return (int)hipGetLastError();
}

int launch_pick(void* stream, const void* store, int nt, int min_fixes, double cutoff, void* work, const Layout& L) {
  if (nt <= 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  int* const cnts = part<int>(work, L.cnts);
  hipLaunchKernelGGL(k_track_pick, dim3(cover(nt, kThreads)), dim3(kThreads), 0, st, (const Track*)store, nt, min_fixes, cutoff,
                     part<int>(work, L.w), cnts);
  compact(st, part<int>(work, L.w), cnts + kCntIn, nt, part<int>(work, L.cnt), cnts + kCntKeys, part<int>(work, L.sel));
  return (int)hipGetLastError();
}

int launch_gather(void* stream, const void* store, int n_max, void* out, void* work, const Layout& L) {
  if (n_max <= 0) return 0;
  hipLaunchKernelGGL(k_track_gather, dim3(cover((long long)n_max * kRowWords, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (const Track*)store,
                     (const int*)part<int>(work, L.sel), (const int*)(part<int>(work, L.cnts) + kCntKeys), (Track*)out);
  return (int)hipGetLastError();
}

}  // namespace adsb_mlat_track_host
