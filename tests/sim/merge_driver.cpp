// merge_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the fleet's merged picture (adsb_stream_planes_merged;
// gr_adsb_amd/csrc/adsb_device.h: k_merge_keys, k_merge_heads, k_merge_emit, with the library's own k_dec_sort_* between
// them) on the SIMT emulator in hipsim.h, on host memory, in the order adsb_hip.hip queues them, over the store and the
// last_seen clocks of expire_driver.cpp's fleet (included unchanged: the emulated fleet step builds what is merged), with
// planes_driver.cpp's selection rule and keys -> count -> sort step.  The host code itself runs only in tests/test_gpu_merge.py.
// Never linked into libadsb_hip.so.
#include "expire_driver.cpp"

extern "C" {

int sim_merge_info_bytes() { return (int)sizeof(MergedInfo); }
// what the seam tests' key arithmetic rests on
void sim_merge_constants(int* chunk, int* threads, int* tile, int* stream_bits, int* addr_bits) {
  *chunk = kMergeChunk; *threads = kThreads; *tile = kSortTile; *stream_bits = kFleetStreamBits; *addr_bits = kFleetAddrBits;
}

// adsb_stream_planes_merged on a fleet of expire_driver.cpp.  streams: null (all), or n_sel indices; rows / info: cap entries
// each, or null.  0; -22: bad indices or cap; -28: cap is too small (*n_out = the rows needed, nothing written); -1: a kernel
// wrote behind one of its arrays; -3: a kernel set the error word, or the counts do not fit.  keys_out (may be null): room for
// every live plane's key -- the sorted keys, *n_keys of them, for tests that place segments across the kernels' seams.
int sim_merge_fleet(void* h, const int* streams, int n_sel, long long cutoff, int grid, int cap, void* rows, void* info, int* n_out,
                    unsigned long long* keys_out, int* n_keys) {
  Fleet& F = *(Fleet*)h;
  Selection S;
  if (!F.ages || cap < 0 || (cap > 0 && !rows && !info) || select_streams(F, streams, &n_sel, &S)) return kInvalid;
  KeyPair K((size_t)F.live_planes);
  Guarded<int> cnt;
  int n = 0;
  const int r = store_keys(F, S, true, cutoff, grid, INT_MAX, K, cnt, &n);
  if (r) return r;
  if (n_keys) *n_keys = n;
  if (n == 0) {
    *n_out = 0;
    return 0;
  }
  const int n_chunks = (n + kMergeChunk - 1) / kMergeChunk;
  if (keys_out) memcpy(keys_out, K.sorted.p(), (size_t)n * 8);
  Guarded<unsigned> counts((size_t)n_chunks + 1, 0xA5);
  hipsim::launch(k_merge_heads, (unsigned)grid, (unsigned)kThreads, (const unsigned long long*)K.sorted.p(), n, counts.p());
  hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, counts.p(), n_chunks + 1);
  if (!counts.ok() || !K.sorted.ok()) return -1;
  const unsigned total = counts.p()[n_chunks];
  if (total == 0 || total > (unsigned)n) return -3;
  *n_out = (int)total;
  if (total > (unsigned)cap) return kNoSpace;
  Guarded<DecRow> rws((size_t)total, 0xA5);
  Guarded<MergedInfo> inf((size_t)total, 0xA5);
  hipsim::launch(k_merge_emit, (unsigned)grid, (unsigned)kThreads, S.a, (const unsigned long long*)K.sorted.p(), n, (const unsigned*)counts.p(),
                 (const long long*)F.st.seen_p(), rows ? rws.p() : (DecRow*)nullptr, info ? inf.p() : (MergedInfo*)nullptr, cnt.p() + 1);
  if (!rws.ok() || !inf.ok() || !counts.ok() || !cnt.ok() || !S.ok() || !K.sorted.ok() || !F.st.ok()) return -1;
  if (cnt.p()[1]) return -3;
  if (rows) memcpy(rows, rws.p(), (size_t)total * sizeof(DecRow));
  if (info) memcpy(info, inf.p(), (size_t)total * sizeof(MergedInfo));
  return 0;
}
}
