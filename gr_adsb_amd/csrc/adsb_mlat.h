// adsb_mlat.h -- the launchers of adsb_mlat.hip (adsb_stream_mlat: adsb_mlat_device.h), for adsb_hip.hip, and the sizing rule
// of the call's work buffer.  Plain pointers only, as adsb_dedup.h: the translation units share no type.  Every call queues
// its kernels on `stream` (a hipStream_t) and returns the hipError_t of the launches as an int (0: queued).  Internal to
// libadsb_hip.so.
#pragma once
#include <stddef.h>

namespace adsb_mlat_host {

constexpr int kEntBytes = 32, kFixBytes = 88, kChunk = 256, kMinRx = 4;

// The work buffer of one call over a carry of nc entries, every part on a 256-byte boundary, all of it sized before the
// first launch: heads <= nc; groups are disjoint and hold at least min_rx used hearings each, so members <= nc and the
// caller states fix_rows > the groups there can be.  aux: one row of aux_row_bytes per fix row behind member_ts
// (adsb_mlat_rule.h); with aux_row_bytes = 0 the part is empty and adds nothing to the total.
struct Layout {
  size_t range, tot_heads, tot_groups;    // int[4] each: {lo, hi}; {0, heads, -, -}; {0, groups, members, -}
  size_t w, cnt, sum;                     // int[nc]: head flags; int[chunks] twice: the compaction's per-chunk arrays
  size_t heads, nrx, gsel, gfirst;        // int[nc] each
  size_t rx;                              // double[3 n_streams]: the receivers' ECEF positions, NaN where none is set
  size_t fixes, member_stream, member_ts; // Fix[fix_rows], int[nc], double[nc]
  size_t aux;                             // aux_row_bytes x fix_rows
  size_t bytes;
};
inline Layout carve(size_t nc, size_t n_streams, size_t fix_rows, size_t aux_row_bytes) {
  Layout L{};
  const size_t chunks = (nc + kChunk - 1) / kChunk + 1;
  const size_t part[15] = {16, 16, 16, nc * 4, chunks * 4, chunks * 4, nc * 4, nc * 4, nc * 4, nc * 4, n_streams * 24,
                           fix_rows * (size_t)kFixBytes, nc * 4, nc * 8, fix_rows * aux_row_bytes};
  size_t* const at[15] = {&L.range, &L.tot_heads, &L.tot_groups, &L.w, &L.cnt, &L.sum, &L.heads, &L.nrx, &L.gsel, &L.gfirst, &L.rx,
                          &L.fixes, &L.member_stream, &L.member_ts, &L.aux};
  size_t off = 0;
  for (int k = 0; k < 15; ++k) { *at[k] = off; off += (part[k] + 255) & ~(size_t)255; }
  L.bytes = off;
  return L;
}
// adsb_stream_mlat's: groups of at least kMinRx, so groups <= nc / kMinRx; no aux rows
inline Layout layout(size_t nc, size_t n_streams) { return carve(nc, n_streams, nc / kMinRx + 1, 0); }

// for the two units' launchers: enough workgroups of a grid-stride kernel to cover `work` units of `per` each, 2048 at the
// most; and a part of the work buffer
inline unsigned cover(long long work, int per) {
  const long long g = (work + per - 1) / per;
  return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
template <class T> T* part(void* work, size_t off) { return (T*)((char*)work + off); }

// carry[nc] -> work: the range of [t_lo, t_hi), the heads in it in carry order, their number in tot_heads[1]
int launch_heads(void* stream, const void* carry, int nc, double t_lo, double t_hi, double window, void* work, const Layout& L);
// heads[nh] -> nrx[nh]; the groups with nrx >= min_rx in gsel / gfirst, their number and members in tot_groups[1], [2]
int launch_groups(void* stream, const void* carry, int nc, int nh, double window, int min_rx, int n_streams, void* work, const Layout& L);
// launch_groups' second half alone, for a caller that wrote nrx[nh] itself (adsb_mlat_rule.h): the compaction with min_w = min_rx
int launch_select(void* stream, int nh, int min_rx, void* work, const Layout& L);
// gsel[ng] -> fixes[ng], member_stream / member_ts
int launch_solve(void* stream, const void* carry, int nc, int ng, double window, int n_streams, void* work, const Layout& L);

}  // namespace adsb_mlat_host
