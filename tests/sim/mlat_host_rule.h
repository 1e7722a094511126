// mlat_host_rule.h -- TEST INFRASTRUCTURE ONLY.  What the two drivers of adsb_stream_mlat's kernels -- tests/sim/mlat_driver.cpp (the
// SIMT emulator, on the CPU) and tests/gpu/mlat_device_driver.hip (the shipped translation unit, on the GPU) -- restate of the
// host's rule in adsb_hip.hip, stated once for both: the parts of the work buffer that adsb_mlat.h's carve() carves and how
// many bytes of each a call may write, the guard bytes between and behind them, and the range checks of the counts that come
// down between the phases (adsb_stream_mlat's -EIO "out of range", the drivers' -5).  Host code only; needs adsb_mlat.h.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

namespace mlat_rule {
namespace mh = adsb_mlat_host;

constexpr unsigned char kGuard = 0xA5;
constexpr size_t kTail = 256;                         // guard bytes behind the last part

// (offset, bytes in use) of every part, in carve()'s order, for a buffer carved with fix_rows rows and aux rows of aux_row_bytes
inline std::vector<std::pair<size_t, size_t>> parts(const mh::Layout& L, size_t nc, size_t n_streams, size_t fix_rows, size_t aux_row_bytes) {
  const size_t chunks = (nc + mh::kChunk - 1) / mh::kChunk + 1;
  return {{L.range, 16}, {L.tot_heads, 16}, {L.tot_groups, 16}, {L.w, nc * 4}, {L.cnt, chunks * 4}, {L.sum, chunks * 4}, {L.heads, nc * 4},
          {L.nrx, nc * 4}, {L.gsel, nc * 4}, {L.gfirst, nc * 4}, {L.rx, n_streams * 24}, {L.fixes, fix_rows * (size_t)mh::kFixBytes},
          {L.member_stream, nc * 4}, {L.member_ts, nc * 8}, {L.aux, fix_rows * aux_row_bytes}};
}
// ... of adsb_mlat.h's layout()
inline std::vector<std::pair<size_t, size_t>> parts(const mh::Layout& L, size_t nc, size_t n_streams) {
  return parts(L, nc, n_streams, nc / mh::kMinRx + 1, 0);
}

// every byte between a part's end and the next part's start (or the tail's end) is still the guard's; raw: L.bytes + kTail
inline bool guards_ok(const unsigned char* raw, size_t raw_bytes, const std::vector<std::pair<size_t, size_t>>& p) {
  for (size_t k = 0; k < p.size(); ++k) {
    const size_t end = k + 1 < p.size() ? p[k + 1].first : raw_bytes;
    if (p[k].first + p[k].second > end) return false;
    for (size_t q = p[k].first + p[k].second; q < end; ++q) if (raw[q] != kGuard) return false;
  }
  return true;
}

// the host's two checks of what comes down, with its own expressions; min_group: the fewest used hearings of a selected group
inline bool heads_in_range(int nh, int nc) { return !(nh < 0 || nh > nc); }
inline bool groups_in_range(int ng, int nm, int nc, int min_rx, int min_group = mh::kMinRx) {
  return !(ng < 0 || ng > nc / min_group || nm < (long long)ng * min_rx || nm > nc);
}

}  // namespace mlat_rule
