// adsb_mlat_track.h -- the launchers of adsb_mlat_track.hip (adsb_stream_mlat_track and the track store's readout and expiry:
// adsb_mlat_track_device.h), for adsb_hip.hip, and the sizing rule of their work buffer.  Plain pointers only, as adsb_mlat.h:
// the translation units share no type.  Every call queues its kernels on `stream` (a hipStream_t) and returns the hipError_t
// of the launches as an int (0: queued).  The key sort is adsb_shared.h's launch_sort.  Internal to libadsb_hip.so.
#pragma once
#include <stddef.h>

#include "adsb_shared.h"

namespace adsb_mlat_track_host {

constexpr int kRowBytes = 96, kRuleBytes = 64, kFixBytes = 88, kAuxBytes = 32, kChunk = 256;
constexpr int kCntWords = 16, kStatWords = 8;         // cnts: int[16] {n, keys | picked, runs, new addresses, ...}; stats: 64-bit words
constexpr int kCntKeys = 1, kCntRuns = 2, kCntNew = 3;
constexpr int kStatUnusable = 0, kStatStale = 1, kStatRejected = 2, kStatTaken = 3, kStatStarted = 4;

// The work buffer of one call over n entries -- an update's fixes, or the store's rows for the readout and expiry -- every
// part on a 256-byte boundary, all of it sized before the first launch: the eligible fixes, the runs and the new addresses
// are each at most n.  hist_bytes: what the sort needs for n pairs (adsb_shared.h: sort_hist_bytes).
struct Layout {
  size_t cnts, stats;                                 // int[kCntWords]; unsigned long long[kStatWords]
  size_t w, cnt;                                      // int[n]: the flags of the compaction at hand; int[chunks]: its per-chunk array
  size_t sel, run_start, run_len, pos, newidx;        // int[n] each
  size_t keys, keys_tmp, vals, vals_tmp, hist;        // 8 n, 8 n, 4 n, 4 n, hist_bytes
  size_t bytes;
};
inline Layout carve(size_t n, size_t hist_bytes) {
  Layout L{};
  const size_t chunks = (n + kChunk - 1) / kChunk + 1;
  const size_t part[14] = {kCntWords * 4, kStatWords * 8, n * 4, chunks * 4, n * 4, n * 4, n * 4, n * 4, n * 4, n * 8, n * 8, n * 4, n * 4, hist_bytes};
  size_t* const at[14] = {&L.cnts, &L.stats, &L.w, &L.cnt, &L.sel, &L.run_start, &L.run_len, &L.pos, &L.newidx, &L.keys, &L.keys_tmp, &L.vals,
                          &L.vals_tmp, &L.hist};
  size_t off = 0;
  for (int k = 0; k < 14; ++k) { *at[k] = off; off += (part[k] + 255) & ~(size_t)255; }
  L.bytes = off;
  return L;
}
inline Layout layout(size_t n) { return carve(n, adsb_shared_host::sort_hist_bytes((int)n)); }

// enough workgroups of a grid-stride kernel to cover `work` units of `per` each, 2048 at the most; and a part of the work buffer
inline unsigned cover(long long work, int per) {
  const long long g = (work + per - 1) / per;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
template <class T> T* part(void* work, size_t off) { return (T*)((char*)work + off); }

// fixes[ng] -> sel[], the unsorted keys and vals of the eligible fixes; their number in cnts[kCntKeys]; the totals cleared
int launch_keys(void* stream, const void* fixes, int ng, void* work, const Layout& L);
// keys[nk] -> the sort, the runs, the find, the merge of store[nt] into next (room for nt + nk rows) and the update.
// aux may be null; rule: kRuleBytes of adsb_mlat_track_rule, in host memory.  cnts[kCntRuns], cnts[kCntNew], stats[] come down.
int launch_update(void* stream, const void* fixes, const void* aux, int nk, const void* rule, const void* store, int nt, void* next, void* work,
                  const Layout& L);
// store[nt] -> w[], sel[] = the rows with n_fixes >= min_fixes and last_ts >= cutoff, in order; their number in cnts[kCntKeys]
int launch_pick(void* stream, const void* store, int nt, int min_fixes, double cutoff, void* work, const Layout& L);
// out[r] = store[sel[r]] for the picked rows (n_max >= their number)
int launch_gather(void* stream, const void* store, int n_max, void* out, void* work, const Layout& L);

}  // namespace adsb_mlat_track_host
