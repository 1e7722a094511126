// adsb_mlat_rule.hip -- the translation unit of adsb_stream_mlat_rule's two kernels (adsb_mlat_rule_device.h) and their
// launchers (adsb_mlat_rule.h).  A unit of its own, so that adsb_mlat.hip's kernels and its resource report are exactly what
// they are without it; it takes adsb_mlat_device.h's device functions without its kernels (ADSB_MLAT_HELPERS_ONLY), and the
// compaction from adsb_mlat.hip's launch_select.  Linked into libadsb_hip.so with the other four.
#include <hip/hip_runtime.h>

#include "adsb_mlat_rule.h"
#define ADSB_MLAT_HELPERS_ONLY
#include "adsb_mlat_device.h"
#include "adsb_mlat_rule_device.h"

namespace adsb_mlat_host {

using namespace adsb_mlat;

static_assert(kAuxBytes == sizeof(Aux) && kFixBytes == sizeof(Fix) && kMinRxAided == 3, "the header's sizes are the device code's");

int launch_groups_rule(void* stream, const void* carry, int nc, int nh, double window, int min_rx, int n_streams, void* work, const RuleLayout& L) {
  if (nh <= 0) return 0;
  hipLaunchKernelGGL(k_mlat_groups_rule, dim3(cover(nh, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)carry, nc,
                     (const int*)part<int>(work, L.heads), (const int*)part<int>(work, L.tot_heads), window,
                     (const double*)part<double>(work, L.rx), n_streams, part<int>(work, L.nrx));
  const int e = (int)hipGetLastError();
  return e ? e : launch_select(stream, nh, min_rx, work, L);
}

int launch_solve_lm(void* stream, const void* carry, int nc, int ng, double window, int n_streams, int flags, double alt_weight, void* work,
                    const RuleLayout& L) {
  if (ng <= 0) return 0;
  hipLaunchKernelGGL(k_mlat_solve_lm, dim3(cover(ng, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)carry, nc,
                     (const int*)part<int>(work, L.heads), (const int*)part<int>(work, L.gsel), (const int*)part<int>(work, L.gfirst),
                     (const int*)part<int>(work, L.tot_groups), window, (const double*)part<double>(work, L.rx), n_streams, flags, alt_weight,
                     part<Fix>(work, L.fixes), part<Aux>(work, L.aux), part<int>(work, L.member_stream), part<double>(work, L.member_ts));
  return (int)hipGetLastError();
}

}  // namespace adsb_mlat_host
