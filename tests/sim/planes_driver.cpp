// planes_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the plane snapshots (gr_adsb_amd/csrc/adsb_device.h: k_planes_tally,
// k_planes_emit, k_planes_store_keys, k_planes_store_emit, and their k_ages_* twins where the last_seen clocks are read too,
// with the library's own k_dec_sort_* between them) on the SIMT emulator in hipsim.h, on host memory, in the order
// adsb_hip.hip's adsb_planes / adsb_stream_planes queue them.  The decoders whose tables are read are those of
// decode_driver.cpp and fleet_driver.cpp, included here unchanged (the fleet's first: it defines the store's compare-and-swap
// before the device header is read).  The host's selection rule and its keys -> count -> sort step have their one emulator
// copy here (select_streams, store_keys), for the snapshots, the expiry (expire_driver.cpp) and the merged picture
// (merge_driver.cpp); the host code itself runs only in tests/test_gpu_planes.py.  Never linked into libadsb_hip.so.
#include "fleet_driver.cpp"
#include "decode_driver.cpp"

namespace {
// adsb_planes / adsb_planes_seen over the addresses [lo, hi).  seen: null (k_planes_emit; rows is there), or the decoder's
// last_seen array (k_ages_emit; rows / seen_out: cap entries each, or null)
int planes_dense(const unsigned long long* table, const void* planes, const long long* seen, unsigned epoch, unsigned lo, unsigned hi, int grid,
                 int cap, void* rows, long long* seen_out, int* n_out) {
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
  Guarded<long long> so((size_t)cap, 0xA5);
  if (total > 0 && !seen) hipsim::launch(k_planes_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned*)counts.p(), cap, out.p());
  if (total > 0 && seen)
    hipsim::launch(k_ages_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned*)counts.p(), cap,
                   rows ? out.p() : (DecRow*)nullptr, seen, seen_out ? so.p() : (long long*)nullptr);
  if (!counts.ok() || !out.ok() || !so.ok()) return -1;
  const size_t k = total < (unsigned)cap ? total : (unsigned)cap;
  if (rows) memcpy(rows, out.p(), k * sizeof(DecRow));
  if (seen_out) memcpy(seen_out, so.p(), k * sizeof(long long));
  return total > (unsigned)cap ? kNoSpace : 0;
}

// The host's selection rule (adsb_hip.hip fleet_selection): streams null selects all, else n_sel >= 0 indices in range and
// strictly ascending -- and what the kernels read of it: generations | selection bitmap | selection list
struct Selection {
  Guarded<unsigned> gen, bits;
  Guarded<int> sel;
  PlanesFleet a{};
  bool ok() const { return gen.ok() && bits.ok() && sel.ok(); }
};
// 0 with *n_sel the streams selected, or -22; S may be null (the rule alone)
int select_streams(Fleet& F, const int* streams, int* n_sel, Selection* S) {
  const size_t ns = F.gen.size();
  if (!streams) *n_sel = (int)ns;
  if (*n_sel < 0) return kInvalid;
  for (int i = 0; streams && i < *n_sel; ++i)
    if (streams[i] < 0 || (size_t)streams[i] >= ns || (i > 0 && streams[i] <= streams[i - 1])) return kInvalid;
  if (!S) return 0;
  S->gen.reset(ns, 0); S->bits.reset((ns + 31) / 32, 0); S->sel.reset((size_t)*n_sel, 0);
  for (size_t s = 0; s < ns; ++s) S->gen.p()[s] = F.gen[s];
  for (int i = 0; streams && i < *n_sel; ++i) {
    S->bits.p()[streams[i] / 32] |= 1u << (streams[i] & 31);
    S->sel.p()[i] = streams[i];
  }
  S->a.s = F.st.view(); S->a.gen = S->gen.p(); S->a.sel_bits = streams ? S->bits.p() : nullptr; S->a.n_streams = (int)ns;
  return 0;
}

// The selected planes' keys, counted, and sorted when there are 1 .. limit of them (adsb_hip.hip fleet_sorted_keys).  merged:
// k_merge_keys (address-major, planes seen before cutoff left out) instead of k_planes_store_keys.  K.cnt: count, error word.
// 0 with *n the keys kept (sorted: in K.sorted); -1: a guard; -3: more keys than the streams count planes, or keys not unique
int store_keys(Fleet& F, Selection& S, bool merged, long long cutoff, int grid, int limit, KeyPair& K, Guarded<int>& cnt, int* n) {
  const int key_cap = (int)F.live_planes;
  cnt.reset(2, 0);
  if (merged)
    hipsim::launch(k_merge_keys, (unsigned)grid, (unsigned)kThreads, S.a, (const long long*)F.st.seen_p(), cutoff, K.keys.p(), key_cap, cnt.p());
  else
    hipsim::launch(k_planes_store_keys, (unsigned)grid, (unsigned)kThreads, S.a, K.keys.p(), key_cap, cnt.p());
  if (!K.keys.ok() || !cnt.ok() || !F.st.ok()) return -1;
  *n = cnt.p()[0];
  if (*n > key_cap) return -3;
  if (*n == 0 || *n > limit) return 0;
  // the keys behind the n kept ones are not part of the sort: what the scatter may not touch
  if (sort_keys(K.keys.p(), K.sorted.p(), *n, 0, kFleetAddrBits + kFleetStreamBits) || !K.ok()) return -1;
  for (int j = 1; j < *n; ++j) if (K.sorted.p()[j - 1] >= K.sorted.p()[j]) return -3;        // unique keys, ascending
  return 0;
}

// adsb_stream_planes / adsb_stream_planes_seen on a fleet.  ages: k_ages_store_emit (rows / seen_out may be null) instead of
// k_planes_store_emit
int planes_fleet(Fleet& F, const int* streams, int n_sel, bool ages, int grid, int cap, void* rows, long long* seen_out, int* first, int* n_out) {
  Selection S;
  if (cap < 0 || (ages && !F.ages) || select_streams(F, streams, &n_sel, &S)) return kInvalid;
  KeyPair K((size_t)F.live_planes);
  Guarded<int> fst((size_t)n_sel + 1, 0xA5), cnt;
  int n = 0;
  const int r = store_keys(F, S, false, 0, grid, cap, K, cnt, &n);
  if (r) return r;
  *n_out = n;
  if (n > cap) return kNoSpace;
  if (n == 0) {
    for (int i = 0; first && i <= n_sel; ++i) first[i] = 0;
    return 0;
  }
  Guarded<DecRow> rws((size_t)n, 0xA5);
  Guarded<long long> so((size_t)n, 0xA5);
  const int* const sel = streams ? S.sel.p() : nullptr;
  if (!ages)
    hipsim::launch(k_planes_store_emit, (unsigned)grid, (unsigned)kThreads, S.a, (const unsigned long long*)K.sorted.p(), n, sel, n_sel, rws.p(),
                   first ? fst.p() : (int*)nullptr, cnt.p() + 1);
  else
    hipsim::launch(k_ages_store_emit, (unsigned)grid, (unsigned)kThreads, S.a, (const unsigned long long*)K.sorted.p(), n, sel, n_sel,
                   rows ? rws.p() : (DecRow*)nullptr, first ? fst.p() : (int*)nullptr, cnt.p() + 1, (const long long*)F.st.seen_p(),
                   seen_out ? so.p() : (long long*)nullptr);
  if (!rws.ok() || !so.ok() || !fst.ok() || !cnt.ok() || !S.ok() || !F.st.ok()) return -1;
  if (cnt.p()[1]) return -3;
  if (rows) memcpy(rows, rws.p(), (size_t)n * sizeof(DecRow));
  if (seen_out) memcpy(seen_out, so.p(), (size_t)n * sizeof(long long));
  if (first) memcpy(first, fst.p(), ((size_t)n_sel + 1) * sizeof(int));
  return 0;
}
}  // namespace

extern "C" {

int sim_planes_chunk() { return kPlanesChunk; }

// adsb_planes over the addresses [lo, hi) (lo a multiple of the chunk, hi even; the product: 0, 2^24).  table / planes: the
// decoder's arrays, indexed by address.  rows: cap rows.  *n_out = the planes in the range.  0; -28: cap is too small -- the
// emit step is run all the same, so that its own bound is tested: rows then holds the first cap rows; -22: a bad range;
// -1: a kernel wrote behind its counts or behind cap rows.
int sim_planes_dense(const unsigned long long* table, const void* planes, unsigned epoch, unsigned lo, unsigned hi, int grid, int cap,
                     void* rows, int* n_out) {
  return planes_dense(table, planes, nullptr, epoch, lo, hi, grid, cap, rows, nullptr, n_out);
}

// adsb_stream_planes on a fleet of fleet_driver.cpp.  streams: null (all), or n_sel indices; first: null, or n_sel + 1 entries.
// 0; -22: indices out of range or not strictly ascending; -28: cap is too small (*n_out = the rows needed, nothing written);
// -1: a kernel wrote behind one of its arrays; -3: a kernel set the error word, or kept more keys than the streams count planes.
int sim_planes_fleet(void* h, const int* streams, int n_sel, int grid, int cap, void* rows, int* first, int* n_out) {
  return planes_fleet(*(Fleet*)h, streams, n_sel, false, grid, cap, rows, nullptr, first, n_out);
}
}
