// merge_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the fleet's merged picture (adsb_stream_planes_merged;
// gr_adsb_amd/csrc/adsb_device.h: k_merge_keys, k_merge_heads, k_merge_emit, with the library's own k_dec_sort_* between
// them) on the SIMT emulator in hipsim.h, on host memory, in the order adsb_hip.hip queues them, over the store and the
// last_seen clocks of expire_driver.cpp's fleet (included unchanged: the emulated fleet step builds what is merged).  The
// host's argument rules are RESTATED here, not shared; the host code itself runs only in tests/test_gpu_merge.py.
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
  AgedFleet& A = *(AgedFleet*)h;
  Fleet& F = A.F;
  const size_t ns = F.gen.size();
  if (!streams) n_sel = (int)ns;
  if (n_sel < 0 || cap < 0 || (cap > 0 && !rows && !info)) return kInvalid;
  for (int i = 0; streams && i < n_sel; ++i)
    if (streams[i] < 0 || (size_t)streams[i] >= ns || (i > 0 && streams[i] <= streams[i - 1])) return kInvalid;
  Guarded<unsigned> gen(ns, 0), bits((ns + 31) / 32, 0);
  Guarded<int> cnt(2, 0);
  for (size_t s = 0; s < ns; ++s) gen.p()[s] = F.gen[s];
  for (int i = 0; streams && i < n_sel; ++i) bits.p()[streams[i] / 32] |= 1u << (streams[i] & 31);
  const long long key_cap = F.live_planes;
  Guarded<unsigned long long> keys((size_t)key_cap, 0xA5, (size_t)kSortTile * 8), sorted((size_t)key_cap, 0xA5, (size_t)kSortTile * 8);
  PlanesFleet a{};
  a.s = F.st.view(); a.gen = gen.p(); a.sel_bits = streams ? bits.p() : nullptr; a.n_streams = (int)ns;
  hipsim::launch(k_merge_keys, (unsigned)grid, (unsigned)kThreads, a, (const long long*)A.seen.p(), cutoff, keys.p(), (int)key_cap, cnt.p());
  if (!keys.ok() || !cnt.ok() || !F.st.ok() || !A.seen.ok()) return -1;
  const int n = cnt.p()[0];
  if (n > key_cap) return -3;
  if (n_keys) *n_keys = n;
  if (n == 0) {
    *n_out = 0;
    return 0;
  }
  const int nblk = (n + kSortTile - 1) / kSortTile, n_chunks = (n + kMergeChunk - 1) / kMergeChunk;
  Guarded<unsigned> hist((size_t)nblk * 16, 0xA5);
  unsigned long long* in = keys.p();
  unsigned long long* out = sorted.p();
  for (int shift = 0; shift < kFleetAddrBits + kFleetStreamBits; shift += 4) {
    hipsim::launch(k_dec_sort_hist, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, n, shift, hist.p());
    hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, hist.p(), nblk * 16);
    hipsim::launch(k_dec_sort_scatter, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, out, n, shift, (const unsigned*)hist.p());
    unsigned long long* x = in; in = out; out = x;
  }
  if (!hist.ok() || !keys.ok() || !sorted.ok()) return -1;
  for (int j = 1; j < n; ++j) if (sorted.p()[j - 1] >= sorted.p()[j]) return -3;        // unique keys, ascending
  if (keys_out) memcpy(keys_out, sorted.p(), (size_t)n * 8);
  Guarded<unsigned> counts((size_t)n_chunks + 1, 0xA5);
  hipsim::launch(k_merge_heads, (unsigned)grid, (unsigned)kThreads, (const unsigned long long*)sorted.p(), n, counts.p());
  hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, counts.p(), n_chunks + 1);
  if (!counts.ok() || !sorted.ok()) return -1;
  const unsigned total = counts.p()[n_chunks];
  if (total == 0 || total > (unsigned)n) return -3;
  *n_out = (int)total;
  if (total > (unsigned)cap) return kNoSpace;
  Guarded<DecRow> rws((size_t)total, 0xA5);
  Guarded<MergedInfo> inf((size_t)total, 0xA5);
  hipsim::launch(k_merge_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned long long*)sorted.p(), n, (const unsigned*)counts.p(),
                 (const long long*)A.seen.p(), rows ? rws.p() : (DecRow*)nullptr, info ? inf.p() : (MergedInfo*)nullptr, cnt.p() + 1);
  if (!rws.ok() || !inf.ok() || !counts.ok() || !cnt.ok() || !gen.ok() || !bits.ok() || !sorted.ok() || !F.st.ok() || !A.seen.ok()) return -1;
  if (cnt.p()[1]) return -3;
  if (rows) memcpy(rows, rws.p(), (size_t)total * sizeof(DecRow));
  if (info) memcpy(info, inf.p(), (size_t)total * sizeof(MergedInfo));
  return 0;
}
}
