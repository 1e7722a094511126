// expire_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the plane ages (ADSB_FLAG_PLANE_AGES; gr_adsb_amd/csrc/adsb_device.h:
// k_ages_fold, k_fleet_fold with FleetArgs::seen set, k_ages_expire, k_ages_emit, k_ages_rehash,
// k_ages_store_emit) on the SIMT emulator in hipsim.h, on host memory, in the order adsb_hip.hip queues them.  The
// decoders are those of decode_driver.cpp and fleet_driver.cpp, included unchanged through planes_driver.cpp; what they do
// without a last_seen array is RESTATED here with one (their DecArgs / FleetArgs are value-initialised: seen is null there).
// The host's argument rules and bookkeeping are restated too; the host code itself runs only in tests/test_gpu_expire.py.
// Never linked into libadsb_hip.so.
#include "planes_driver.cpp"

#include <climits>

namespace {
// a fleet of fleet_driver.cpp and the last_seen clocks beside its store's slots
struct AgedFleet {
  Fleet F;
  Guarded<long long> seen;
};

// fleet_rehash of a flagged context: k_ages_rehash; cutoffs ([n_streams]) make it an expiry.  0, -1 (a guard), -3
int rehash_seen(AgedFleet& A, long long new_cap, int grid, bool renumber, const long long* cutoffs, long long* n_removed) {
  Fleet& F = A.F;
  const size_t ns = F.gen.size();
  Store to;
  to.build(new_cap);
  Guarded<long long> to_seen((size_t)new_cap, 0xA5), cut(ns, 0);
  Guarded<unsigned> gen(ns, 0);
  Guarded<FleetCount> removed(ns, 0);
  Guarded<int> err(1, 0);
  for (size_t s = 0; s < ns; ++s) gen.p()[s] = F.gen[s];
  for (size_t s = 0; cutoffs && s < ns; ++s) cut.p()[s] = cutoffs[s];
  FleetAges g{};
  g.from_seen = A.seen.p(); g.to_seen = to_seen.p();
  if (cutoffs) { g.cutoffs = cut.p(); g.removed = removed.p(); }
  hipsim::launch(k_ages_rehash, (unsigned)grid, (unsigned)kThreads, F.st.view(), to.view(), (const unsigned*)gen.p(), (int)ns,
                 renumber ? 1 : 0, err.p(), g);
  if (!F.st.ok() || !to.ok() || !gen.ok() || !err.ok() || !A.seen.ok() || !to_seen.ok() || !cut.ok() || !removed.ok()) return -1;
  if (err.p()[0]) return -3;
  F.st = std::move(to);
  A.seen = std::move(to_seen);
  long long total = 0;
  for (size_t s = 0; s < ns; ++s) {
    const FleetCount r = removed.p()[s];
    if (r.slots != r.planes) return -3;
    F.slots[s] -= r.slots; F.planes[s] -= r.planes;
    F.live_slots -= r.slots; F.live_planes -= r.planes;
    total += r.planes;
  }
  if (n_removed) *n_removed = total;
  F.used = F.live_slots;
  if (renumber) F.call = 1;
  return 0;
}
}  // namespace

extern "C" {

// ---- one decoder ---------------------------------------------------------------------------------------------------------------
// sim_dec_pdus with the last_seen array (2^24 int64, never cleared: any bytes at first); seen null: as sim_dec_pdus
int sim_exp_dec_pdus(unsigned char* bits14, const double* ts, int n, int grid, unsigned long long* table, void* st, void* planes,
                     long long* seen, unsigned epoch, unsigned long long pass, int fec, int all, void* rows) {
  std::vector<unsigned char> ok((size_t)n);
  std::vector<unsigned long long> keys((size_t)n + kSortTile, kGuard), sorted((size_t)n + kSortTile, kGuard);
  hipsim::launch(k_dec_pdu_flags, (unsigned)grid, (unsigned)kThreads, (const unsigned char*)bits14, ok.data(), n);
  if (fec) hipsim::launch(k_fec_slices, (unsigned)grid, (unsigned)kThreads, bits14, ok.data(), n);
  AirArgs a{};
  a.bits14 = bits14; a.ok = ok.data(); a.cap = n; a.table = table; a.st = (AirState*)st; a.pass = pass << 32; a.fec = fec;
  hipsim::launch(k_air_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_air_cond, 1u, 64u, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  DecArgs d{};
  d.air = a; d.ts = ts; d.planes = (Plane*)planes; d.epoch = epoch; d.all = all; d.keys = keys.data(); d.sorted = sorted.data();
  d.rows = (DecRow*)rows; d.seen = seen;
  hipsim::launch(k_dec_classify, (unsigned)grid, (unsigned)kThreads, d);
  if (sort_keys(keys, sorted, n)) return -1;
  for (int i = 0; i < n; ++i)
    if (sorted[i] != kDecNoKey && (unsigned)sorted[i] >= (unsigned)n) return -2;
  if (seen) hipsim::launch(k_ages_fold, (unsigned)grid, (unsigned)kThreads, d);         // launch_dec's choice
  else hipsim::launch(k_dec_fold, (unsigned)grid, (unsigned)kThreads, d);
  return 0;
}

// adsb_planes_expire over the addresses [lo, hi) (as sim_planes_dense).  0; -22: a bad range; -1: the counter's guard
int sim_exp_dense_expire(unsigned long long* table, void* planes, const long long* seen, unsigned epoch, unsigned lo, unsigned hi,
                         int grid, long long cutoff, long long* n_removed) {
  if (lo % kPlanesChunk || (hi & 1u) || hi < lo || hi > (1u << 24)) return kInvalid;
  PlanesExpire a{};
  a.table = table; a.planes = (Plane*)planes; a.seen = seen; a.epoch = epoch; a.lo = lo; a.hi = hi; a.cutoff = cutoff;
  Guarded<unsigned long long> cnt(1, 0);
  hipsim::launch(k_ages_expire, (unsigned)grid, (unsigned)kThreads, a, cnt.p());
  if (!cnt.ok()) return -1;
  *n_removed = (long long)cnt.p()[0];
  return 0;
}

// adsb_planes_seen over [lo, hi): sim_planes_dense with k_ages_emit; rows / seen_out: cap entries each, or null
int sim_exp_dense_seen(const unsigned long long* table, const void* planes, const long long* seen, unsigned epoch, unsigned lo,
                       unsigned hi, int grid, int cap, void* rows, long long* seen_out, int* n_out) {
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
  if (total > 0)
    hipsim::launch(k_ages_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned*)counts.p(), cap,
                   rows ? out.p() : (DecRow*)nullptr, seen, seen_out ? so.p() : (long long*)nullptr);
  if (!counts.ok() || !out.ok() || !so.ok()) return -1;
  const size_t k = total < (unsigned)cap ? total : (unsigned)cap;
  if (rows) memcpy(rows, out.p(), k * sizeof(DecRow));
  if (seen_out) memcpy(seen_out, so.p(), k * sizeof(long long));
  return total > (unsigned)cap ? kNoSpace : 0;
}

// ---- the fleet -----------------------------------------------------------------------------------------------------------------
// The handle's first member is fleet_driver.cpp's Fleet: sim_fleet_set_start / _set_gen / _set_call / _get_call / _stats /
// _taken and sim_planes_fleet take it as it is.  sim_fleet_call, sim_fleet_reset and sim_fleet_close do NOT (no last_seen).
void* sim_exp_fleet_open(int n_streams, long long slots, int fec, int all) {
  AgedFleet* A = new AgedFleet();
  Fleet* F = &A->F;
  F->fec = fec; F->all = all;
  F->start.assign((size_t)n_streams, 0.0); F->gen.assign((size_t)n_streams, 0u);
  F->slots.assign((size_t)n_streams, 0); F->planes.assign((size_t)n_streams, 0);
  long long cap = kMinCap;
  while (cap < slots) cap *= 2;
  F->st.build(cap);
  A->seen.reset((size_t)cap, 0xA5);
  return A;
}
void sim_exp_fleet_close(void* h) { delete (AgedFleet*)h; }
int sim_exp_fleet_reset(void* h, int stream) {
  AgedFleet& A = *(AgedFleet*)h;
  Fleet& F = A.F;
  const size_t s = (size_t)stream;
  F.live_slots -= F.slots[s]; F.live_planes -= F.planes[s];
  F.slots[s] = F.planes[s] = 0;
  if (F.gen[s] < kFleetGenMax) { ++F.gen[s]; return 0; }
  F.gen[s] = ~0u;
  const int r = rehash_seen(A, F.st.cap, 3, false, nullptr, nullptr);
  F.gen[s] = 0;
  return r;
}
// the slot of (stream, addr) in its current generation, -1 if none (for tests that build probe clusters)
long long sim_exp_fleet_slot_of(void* h, int stream, unsigned addr) {
  Fleet& F = ((AgedFleet*)h)->F;
  const unsigned long long key = ((unsigned long long)F.gen[(size_t)stream] << (kFleetAddrBits + kFleetStreamBits)) |
                                 ((unsigned long long)(unsigned)stream << kFleetAddrBits) | addr;
  bool claimed = false;
  const unsigned s = fleet_slot(F.st.view(), key, false, &claimed);
  return s == kFleetNone ? -1 : (long long)s;
}
// the home slot of (stream, addr) in a store of cap slots
unsigned sim_exp_fleet_home(void* h, int stream, unsigned addr, long long cap) {
  Fleet& F = ((AgedFleet*)h)->F;
  const unsigned long long key = ((unsigned long long)F.gen[(size_t)stream] << (kFleetAddrBits + kFleetStreamBits)) |
                                 ((unsigned long long)(unsigned)stream << kFleetAddrBits) | addr;
  return fleet_hash(key) & (unsigned)(cap - 1);
}

// sim_fleet_call with the last_seen array (return values as there)
int sim_exp_fleet_call(void* h, const unsigned char* bits14, const double* ts, const int* stream, int n, int grid, void* rows_out) {
  AgedFleet& A = *(AgedFleet*)h;
  Fleet& F = A.F;
  if (n <= 0) return 0;
  for (int i = 0; i < n; ++i) if (stream[i] < 0 || (size_t)stream[i] >= F.gen.size()) return -5;
  std::vector<int> order_of_stream(F.gen.size(), -1), item_stream;
  for (int i = 0; i < n; ++i)
    if (order_of_stream[(size_t)stream[i]] < 0) { order_of_stream[(size_t)stream[i]] = (int)item_stream.size(); item_stream.push_back(stream[i]); }
  const int n_items = (int)item_stream.size();
  std::vector<std::vector<int>> members((size_t)n_items);
  for (int i = 0; i < n; ++i) members[(size_t)order_of_stream[(size_t)stream[i]]].push_back(i);
  std::vector<int> src;
  Guarded<FleetItem> items((size_t)n_items + 1, 0);
  for (int k = 0; k < n_items; ++k) {
    const size_t s = (size_t)item_stream[(size_t)k];
    FleetItem& it = items.p()[k];
    it.first = (int)src.size(); it.stream = (int)s;
    it.base = ((unsigned long long)F.gen[s] << (kFleetAddrBits + kFleetStreamBits)) | ((unsigned long long)s << kFleetAddrBits);
    it.start = (double)(long long)F.start[s];
    src.insert(src.end(), members[(size_t)k].begin(), members[(size_t)k].end());
  }
  items.p()[n_items].first = n; items.p()[n_items].stream = -1;
  Guarded<unsigned char> b14((size_t)n * 14, 0), ok((size_t)n, 0);
  for (int t = 0; t < n; ++t) memcpy(b14.p() + (size_t)t * 14, bits14 + (size_t)src[(size_t)t] * 14, 14);
  hipsim::launch(k_dec_pdu_flags, (unsigned)grid, (unsigned)kThreads, (const unsigned char*)b14.p(), ok.p(), n);
  if (F.fec) hipsim::launch(k_fec_slices, (unsigned)grid, (unsigned)kThreads, b14.p(), ok.p(), n);
  if (!b14.ok() || !ok.ok()) return -1;
  Guarded<Rec> recs((size_t)n, 0);
  for (int t = 0; t < n; ++t) {
    const unsigned char* p = b14.p() + (size_t)t * 14;
    const unsigned o = ok.p()[t];
    unsigned long long w2 = 0, w3 = 0;
    for (int k = 0; k < 8; ++k) w2 |= (unsigned long long)p[k] << (8 * k);
    for (int k = 0; k < 6; ++k) w3 |= (unsigned long long)p[8 + k] << (8 * k);
    const unsigned fl = (o & 0xE1u) | ((o & 6u) << 13);
    Rec& r = recs.p()[t];
    const size_t s = (size_t)stream[(size_t)src[(size_t)t]];
    r.w[0] = (unsigned long long)((long long)ts[(size_t)src[(size_t)t]] - (long long)F.start[s]);
    r.w[1] = 0; r.w[2] = w2; r.w[3] = w3 | ((unsigned long long)fl << 48);
  }
  const bool renumber = F.call >= 0xFFFFFFFEull;
  if ((F.used + n) * 2 > F.st.cap || renumber) {
    const long long old_cap = F.st.cap;
    long long cap = old_cap;
    while ((F.live_slots + n) * 2 > cap) cap *= 2;
    if (cap > kMaxCap) return -4;
    const int r = rehash_seen(A, cap, grid, renumber, nullptr, nullptr);
    if (r) return r;
    if (cap > old_cap) F.grows++;
  }
  Guarded<FleetCount> count((size_t)n_items, 0);
  Guarded<int> ncond((size_t)n_items + 1, 0), err(1, 0);
  Guarded<unsigned long long> keys((size_t)n, 0xA5, (size_t)kSortTile * 8), sorted((size_t)n, 0xA5, (size_t)kSortTile * 8);
  Guarded<double> tsd((size_t)n, 0xA5);
  Guarded<DecRow> rows((size_t)n, 0xA5);
  FleetArgs a{};
  a.recs = recs.p(); a.n = n; a.n_items = n_items; a.items = items.p(); a.count = count.p(); a.ncond = ncond.p(); a.error = err.p();
  a.s = F.st.view(); a.call = F.call << 32; a.fec = F.fec; a.all = F.all; a.fs = 1.0;
  a.keys = keys.p(); a.sorted = sorted.p(); a.ts = tsd.p(); a.rows = rows.p(); a.seen = A.seen.p();
  auto guards = [&]() {
    return recs.ok() && items.ok() && count.ok() && ncond.ok() && err.ok() && keys.ok() && sorted.ok() && tsd.ok() && rows.ok() &&
           F.st.ok() && A.seen.ok();
  };
  hipsim::launch(k_fleet_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_fleet_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_fleet_cond, (unsigned)n_items, 64u, a);
  hipsim::launch(k_fleet_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  hipsim::launch(k_fleet_classify, (unsigned)grid, (unsigned)kThreads, a);
  if (!guards()) return -1;
  {
    const int nblk = (n + kSortTile - 1) / kSortTile;
    Guarded<unsigned> hist((size_t)nblk * 16, 0xA5);
    unsigned long long* in = keys.p();
    unsigned long long* out = sorted.p();
    for (int shift = 32; shift < 60; shift += 4) {
      hipsim::launch(k_dec_sort_hist, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, n, shift, hist.p());
      hipsim::launch(k_dec_sort_scan, 1u, (unsigned)kThreads, hist.p(), nblk * 16);
      hipsim::launch(k_dec_sort_scatter, (unsigned)nblk, (unsigned)kThreads, (const unsigned long long*)in, out, n, shift,
                     (const unsigned*)hist.p());
      unsigned long long* x = in; in = out; out = x;
    }
    if (!hist.ok() || !guards()) return -1;
  }
  for (int i = 0; i < n; ++i) {
    const unsigned long long k = sorted.p()[i];
    if (k != kDecNoKey && ((unsigned)k >= (unsigned)n || (k >> 32) >= (unsigned long long)F.st.cap)) return -2;
  }
  hipsim::launch(k_fleet_fold, (unsigned)((n + kThreads - 1) / kThreads), (unsigned)kThreads, a);
  if (!guards()) return -1;
  if (err.p()[0]) return -3;
  for (int k = 0; k < n_items; ++k) {
    const size_t s = (size_t)item_stream[(size_t)k];
    const FleetCount c = count.p()[k];
    F.slots[s] += c.slots; F.planes[s] += c.planes;
    F.live_slots += c.slots; F.live_planes += c.planes; F.used += c.slots;
  }
  F.call++;
  for (int t = 0; t < n; ++t) memcpy((char*)rows_out + (size_t)src[(size_t)t] * sizeof(DecRow), &rows.p()[t], sizeof(DecRow));
  return 0;
}

// adsb_stream_planes_expire: streams null (all; cutoffs[n_streams]) or n_sel strictly ascending indices (cutoffs[n_sel]).
// 0; -22: bad indices or cutoffs missing; -1 / -3 as the rehash
int sim_exp_fleet_expire(void* h, const int* streams, int n_sel, const long long* cutoffs, int grid, long long* n_removed) {
  AgedFleet& A = *(AgedFleet*)h;
  const size_t ns = A.F.gen.size();
  if (!streams) n_sel = (int)ns;
  if (n_sel < 0 || (n_sel > 0 && !cutoffs)) return kInvalid;
  for (int i = 0; streams && i < n_sel; ++i)
    if (streams[i] < 0 || (size_t)streams[i] >= ns || (i > 0 && streams[i] <= streams[i - 1])) return kInvalid;
  std::vector<long long> cut(ns, LLONG_MIN);
  for (int i = 0; i < n_sel; ++i) cut[streams ? (size_t)streams[i] : (size_t)i] = cutoffs[i];
  return rehash_seen(A, A.F.st.cap, grid, false, cut.data(), n_removed);
}

// adsb_stream_planes_seen: sim_planes_fleet with k_ages_store_emit; rows / seen_out may be null
int sim_exp_fleet_seen(void* h, const int* streams, int n_sel, int grid, int cap, void* rows, long long* seen_out, int* first,
                       int* n_out) {
  AgedFleet& A = *(AgedFleet*)h;
  Fleet& F = A.F;
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
  Guarded<DecRow> rws((size_t)n, 0xA5);
  Guarded<long long> so((size_t)n, 0xA5);
  hipsim::launch(k_ages_store_emit, (unsigned)grid, (unsigned)kThreads, a, (const unsigned long long*)sorted.p(), n,
                 streams ? (const int*)sel.p() : (const int*)nullptr, n_sel, rows ? rws.p() : (DecRow*)nullptr,
                 first ? fst.p() : (int*)nullptr, cnt.p() + 1, (const long long*)A.seen.p(), seen_out ? so.p() : (long long*)nullptr);
  if (!rws.ok() || !so.ok() || !fst.ok() || !cnt.ok() || !gen.ok() || !bits.ok() || !sel.ok() || !F.st.ok() || !A.seen.ok()) return -1;
  if (cnt.p()[1]) return -3;
  if (rows) memcpy(rows, rws.p(), (size_t)n * sizeof(DecRow));
  if (seen_out) memcpy(seen_out, so.p(), (size_t)n * sizeof(long long));
  if (first) memcpy(first, fst.p(), ((size_t)n_sel + 1) * sizeof(int));
  return 0;
}
}
