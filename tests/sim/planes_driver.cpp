// planes_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the plane snapshots (gr_adsb_amd/csrc/adsb_device.h: k_planes_tally,
// k_planes_emit, k_planes_store_keys, k_planes_store_emit, with the library's own k_dec_sort_* between them) on the SIMT
// emulator in hipsim.h, on host memory, in the order adsb_hip.hip's adsb_planes / adsb_stream_planes queue them.  The decoders
// whose tables are read are those of decode_driver.cpp and fleet_driver.cpp, included here unchanged (the fleet's first: it
// defines the store's compare-and-swap before the device header is read).  The host's argument rules are RESTATED here, not
// shared; the host code itself runs only in tests/test_gpu_planes.py.  Never linked into libadsb_hip.so.
#include "fleet_driver.cpp"
#include "decode_driver.cpp"

namespace {
constexpr int kNoSpace = -28, kInvalid = -22;
}

extern "C" {

int sim_planes_chunk() { return kPlanesChunk; }

// adsb_planes over the addresses [lo, hi) (lo a multiple of the chunk, hi even; the product: 0, 2^24).  table / planes: the
// decoder's arrays, indexed by address.  rows: cap rows.  *n_out = the planes in the range.  0; -28: cap is too small -- the
// emit step is run all the same, so that its own bound is tested: rows then holds the first cap rows; -22: a bad range;
// -1: a kernel wrote behind its counts or behind cap rows.
int sim_planes_dense(const unsigned long long* table, const void* planes, unsigned epoch, unsigned lo, unsigned hi, int grid, int cap,
                     void* rows, int* n_out) {
  if (lo % kPlanesChunk || (hi & 1u) || hi < lo || hi > (1u << 24) || cap < 0) return kInvalid;
  PlanesDense a{};
  a.table = table; a.planes = (const Plane*)planes; a.epoch = epoch; a.lo = lo; a.hi = hi;
  const unsigned n_chunks = (hi - lo + kPlanesChunk - 1u) / kPlanesChunk;
  Guarded<unsigned> counts((size_t)n_chunks + 1, 0xA5);
  hipsim::launch(k_planes_tally, (unsigned)grid, (unsigned)kThreads, a, counts.p());
  hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, counts.p(), (int)n_chunks + 1);
  if (!counts.ok()) return -1;
  const unsigned total = counts.p()[n_chunks];
  *n_out = (int)total;
  Guarded<DecRow> out((size_t)cap, 0xA5);
  if (total > 0) hipsim::launch(k_planes_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned*)counts.p(), cap, out.p());
  if (!counts.ok() || !out.ok()) return -1;
  memcpy(rows, out.p(), (size_t)(total < (unsigned)cap ? total : (unsigned)cap) * sizeof(DecRow));
  return total > (unsigned)cap ? kNoSpace : 0;
}

// adsb_stream_planes on a fleet of fleet_driver.cpp.  streams: null (all), or n_sel indices; first: null, or n_sel + 1 entries.
// 0; -22: indices out of range or not strictly ascending; -28: cap is too small (*n_out = the rows needed, nothing written);
// -1: a kernel wrote behind one of its arrays; -3: a kernel set the error word, or kept more keys than the streams count planes.
int sim_planes_fleet(void* h, const int* streams, int n_sel, int grid, int cap, void* rows, int* first, int* n_out) {
  Fleet& F = *(Fleet*)h;
  const size_t ns = F.gen.size();
  if (!streams) n_sel = (int)ns;
  if (n_sel < 0 || cap < 0) return kInvalid;
  for (int i = 0; streams && i < n_sel; ++i)
    if (streams[i] < 0 || (size_t)streams[i] >= ns || (i > 0 && streams[i] <= streams[i - 1])) return kInvalid;
  Guarded<unsigned> gen(ns, 0), bits((ns + 31) / 32, 0);
  Guarded<int> sel((size_t)n_sel, 0), fst((size_t)n_sel + 1, 0xA5), cnt(2, 0);
  for (size_t s = 0; s < ns; ++s) gen.p()[s] = F.gen[s];
  for (int i = 0; streams && i < n_sel; ++i) {
    bits.p()[streams[i] / 32] |= 1u << (streams[i] & 31);
    sel.p()[i] = streams[i];
  }
  const long long key_cap = F.live_planes;
  Guarded<unsigned long long> keys((size_t)key_cap, 0xA5, (size_t)kSortTile * 8), sorted((size_t)key_cap, 0xA5, (size_t)kSortTile * 8);
  PlanesFleet a{};
  a.s = F.st.view(); a.gen = gen.p(); a.sel_bits = streams ? bits.p() : nullptr; a.n_streams = (int)ns;
  hipsim::launch(k_planes_store_keys, (unsigned)grid, (unsigned)kThreads, a, keys.p(), (int)key_cap, cnt.p());
  if (!keys.ok() || !cnt.ok() || !F.st.ok()) return -1;
  const int n = cnt.p()[0];
  if (n > key_cap) return -3;
  *n_out = n;
  if (n > cap) return kNoSpace;
  if (n == 0) {
    for (int i = 0; first && i <= n_sel; ++i) first[i] = 0;
    return 0;
  }
  // the keys behind the n kept ones are not part of the sort: what the scatter may not touch
  const int nblk = (n + kSortTile - 1) / kSortTile;
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
  Guarded<DecRow> rws((size_t)n, 0xA5);
  hipsim::launch(k_planes_store_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned long long*)sorted.p(), n,
                 streams ? (const int*)sel.p() : (const int*)nullptr, n_sel, rws.p(), first ? fst.p() : (int*)nullptr, cnt.p() + 1);
  if (!rws.ok() || !fst.ok() || !cnt.ok() || !gen.ok() || !bits.ok() || !sel.ok() || !F.st.ok()) return -1;
  if (cnt.p()[1]) return -3;
  memcpy(rows, rws.p(), (size_t)n * sizeof(DecRow));
  if (first) memcpy(first, fst.p(), ((size_t)n_sel + 1) * sizeof(int));
  return 0;
}
}
