// adsb_softfec_batch.h -- the launcher of adsb_softfec_batch.hip (ADSB_FLAG_FEC_SOFT_BATCH's kernel: adsb_softfec_batch_device.h),
// for adsb_hip.hip.  Plain pointers only, as adsb_softfec.h: the translation units share no type.  The call queues one kernel
// on `stream` (a hipStream_t) and returns the hipError_t of the launch as an int (0: queued).  Internal to libadsb_hip.so.
#pragma once

namespace adsb_softfec_batch_host {

constexpr int kItemBytes = 32, kRowBytes = 8, kRuleBytes = 16, kRecWords = 4;

// One item of the table the host writes (device memory when launched): the item's samples as its k_batch workgroup read them.
struct Item { const void* data; long long n; long long origin; long long reserved; };
static_assert(sizeof(Item) == kItemBytes, "32 bytes per item");

// The packed list of one batch pass, in place, behind k_fec: out[out_cap] records of four words, item i's in
// [first[i], first[i + 1]) (first[n_items + 1] as k_batch_pack wrote it: device-visible), the pinned mirror of the first
// host_cap records (null: none), rows[out_cap].  One workgroup per item.  mode: ADSB_FMT_*; scale / sps: the context's.
// rule: kRuleBytes of adsb_soft_fec_rule, in host memory.
int launch_items(void* stream, int n_items, int mode, const void* items, const int* first, float scale, int sps, const void* rule,
                 void* out, int out_cap, void* host_out, int host_cap, void* rows);

}  // namespace adsb_softfec_batch_host
