// adsb_softfec_batch.hip -- the translation unit of the batch passes' soft-decision CRC repair: k_soft_fec_batch
// (adsb_softfec_batch_device.h) and its launcher (adsb_softfec_batch.h).  An eighth unit, so that the kernels of the other
// seven and their resource reports are exactly what they are without it.  Linked into libadsb_hip.so.
#include <hip/hip_runtime.h>

#include <string.h>

#if defined(__HIP__)
#include "adsb_env_hip.h"
#endif   // (a host compiler gets the SIMT emulator's environment with its <hip/hip_runtime.h>)
#include "adsb_softfec_batch.h"
#include "adsb_softfec_batch_device.h"

namespace adsb_softfec_batch_host {

using namespace adsb_softfec_batch;

static_assert(sizeof(Item) == sizeof(adsb_softfec_batch::Item) && offsetof(Item, n) == offsetof(adsb_softfec_batch::Item, n) &&
              offsetof(Item, origin) == offsetof(adsb_softfec_batch::Item, origin) && kRuleBytes == sizeof(Rule),
              "the header's table and sizes are the device code's");

namespace {
template <int MODE>
void launch_mode(hipStream_t st, int n_items, const adsb_softfec_batch::Item* items, const int* first, float scale, int sps, const Rule& R,
                 unsigned long long* out, int out_cap, unsigned long long* host_out, int host_cap, unsigned long long* rows) {
  hipLaunchKernelGGL((k_soft_fec_batch<MODE>), dim3((unsigned)n_items), dim3(kThreads), 0, st, items, first, scale, sps, R, out, out_cap,
                     host_out, host_cap, rows);
}
}  // namespace

int launch_items(void* stream, int n_items, int mode, const void* items, const int* first, float scale, int sps, const void* rule,
                 void* out, int out_cap, void* host_out, int host_cap, void* rows) {
  if (n_items <= 0 || out_cap <= 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  Rule R;
  memcpy(&R, rule, sizeof R);
  const adsb_softfec_batch::Item* const it = (const adsb_softfec_batch::Item*)items;
  unsigned long long* const o = (unsigned long long*)out;
  unsigned long long* const h = (unsigned long long*)host_out;
  unsigned long long* const r = (unsigned long long*)rows;
  switch (mode) {
    case 0: launch_mode<0>(st, n_items, it, first, scale, sps, R, o, out_cap, h, h ? host_cap : 0, r); break;
    case 1: launch_mode<1>(st, n_items, it, first, scale, sps, R, o, out_cap, h, h ? host_cap : 0, r); break;
    case 2: launch_mode<2>(st, n_items, it, first, scale, sps, R, o, out_cap, h, h ? host_cap : 0, r); break;
    case 3: launch_mode<3>(st, n_items, it, first, scale, sps, R, o, out_cap, h, h ? host_cap : 0, r); break;
    case 4: launch_mode<4>(st, n_items, it, first, scale, sps, R, o, out_cap, h, h ? host_cap : 0, r); break;
    default: return 1;   // hipErrorInvalidValue
  }
  return (int)hipGetLastError();
}

}  // namespace adsb_softfec_batch_host
