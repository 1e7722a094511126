// adsb_softfec_batch_device.h -- device code of the soft-decision CRC repair for the batch passes (ADSB_FLAG_FEC_SOFT_BATCH;
// include/adsb_hip.h: SOFT REPAIR, IN A BATCH).  adsb_process_batch* and adsb_process_stream_batch* leave ONE packed record list
// for all items (k_batch_pack), while the samples a record was sliced from are its own item's: a batch item's buffer is the
// caller's, a stream item's is [carry | chunk] in the library's staging buffer.  The kernel here is k_soft_fec told which item
// a packed record belongs to; the rule, the row and the repaired flags are adsb_softfec_device.h's, included and not restated.
//
//   k_soft_fec_batch<MODE>   the packed list of a batch pass, in place, behind k_fec (device list and pinned mirror)
//
// Cold code in k_soft_fec's style: workgroup i = item i, its four wavefronts stride the item's records packed[first[i] ..
// first[i + 1]) with first[] as k_batch_pack wrote it; an item the host runs itself has an empty range.  A record that does not
// qualify leaves after one flag read.  One 8-byte row (adsb_soft_fix) per packed record, zero where the rule does not apply.
// 64 bytes of LDS per wavefront, no scratch.  Plain C++ vector stores only.
//
// Device code only, as adsb_softfec_device.h: the includer provides the HIP device environment.
#pragma once

#ifndef ADSB_SOFTFEC_RULE_ONLY
#define ADSB_SOFTFEC_RULE_ONLY   // k_soft_fec_slices is not a template: it belongs to adsb_softfec.hip alone
#endif
#include "adsb_softfec_device.h"

namespace adsb_softfec_batch {

using adsb_softfec::kMaxWeak;
using adsb_softfec::kThreads;
using adsb_softfec::kWaves;
using adsb_softfec::Rule;

// One item's samples as its own k_batch workgroup read them (Plan: d_data, n, origin); the host writes the table.
struct Item { const void* data; long long n; long long origin; long long reserved; };
static_assert(sizeof(Item) == 32, "the host's table is 32 bytes per item");

// out: the packed list, four words per record, out_cap slots; first[n_items + 1]: the items' ranges in it, ascending; host_out:
// the pinned mirror of the first host_cap records (may be null); rows[out_cap].  grid = n_items.
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_soft_fec_batch(const Item* items, const int* first, float scale, int sps, Rule R,
                                                             unsigned long long* out, int out_cap, unsigned long long* host_out,
                                                             int host_cap, unsigned long long* rows) {
  __shared__ unsigned s_syn[kWaves][kMaxWeak];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int item = (int)blockIdx.x;
  int lo = first[item], hi = first[item + 1];
  if (lo < 0) lo = 0;
  if (hi > out_cap) hi = out_cap;
  if (lo >= hi) return;                                   // (an empty item's data pointer is never read)
  const Item it = items[item];
  for (int t = lo + wave; t < hi; t += kWaves) {
    unsigned long long w3 = out[4ll * t + 3];
    const unsigned fl = (unsigned)(w3 >> 48);
    unsigned long long row = 0ull;
    if ((fl & adsb::kDemod) && !(fl & (adsb::kParityOk | adsb::kFecDf)) && ((1u << ((fl >> adsb::kDfShift) & 31u)) & adsb::kDfPiSet)) {
      unsigned long long w2 = out[4ll * t + 2];
      const long long p = (long long)out[4ll * t] - it.origin;         // local to the record's OWN item
      if (adsb_softfec::soft_repair<MODE>(it.data, it.n, scale, sps, p, w2, w3, R, lane, s_syn[wave], row)) {
        w3 = (w3 & 0xFFFFFFFFFFFFull) | ((unsigned long long)adsb_softfec::repaired_flags(fl, w2, w3 & 0xFFFFFFFFFFFFull) << 48);
        if (lane == 0) {
          out[4ll * t + 2] = w2; out[4ll * t + 3] = w3;
          if (t < host_cap) { host_out[4ll * t + 2] = w2; host_out[4ll * t + 3] = w3; }
        }
      }
    }
    if (lane == 0) rows[t] = row;
  }
}

}  // namespace adsb_softfec_batch
