// fleet_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the per-stream decoders (ADSB_FLAG_STREAM_DECODE; gr_adsb_amd/csrc/
// adsb_device.h: k_fleet_announce, k_fleet_verdict, k_fleet_cond, k_fleet_classify, k_dec_sort_*, k_fleet_fold,
// k_fleet_rehash, and with the last_seen clocks of ADSB_FLAG_PLANE_AGES beside the store k_ages_rehash) on the SIMT emulator
// in hipsim.h, on host memory, in the order adsb_hip.hip's fleet_step queues them, with the host's growth rule in front
// (fleet_rehash) and its per-stream bookkeeping behind.  The emulator's one copy of them: rehash and decode_step below serve
// the plain fleet, the fleet with ages (expire_driver.cpp) and the shared decoder (shared_driver.cpp).  The host's own
// fleet_step / fleet_rehash / fleet_reset_stream run only in tests/test_gpu_stream_decode.py.  This driver's clock is whole
// seconds at fs = 1, so start + (double)offset / fs with fractional starts is a GPU test's matter too.
// Never linked into libadsb_hip.so.
#include "hipsim.h"

// The store's compare-and-swap for the emulator: fibers switch only at barriers and wave intrinsics, so this
// read-compare-write is indivisible.  It counts the claims, which the per-item counters of the kernels have to add up to.
static long long g_fleet_claims = 0;
inline unsigned long long fleet_driver_cas(unsigned long long* p, unsigned long long e, unsigned long long d) {
  const unsigned long long o = *p;
  if (o == e) { *p = d; ++g_fleet_claims; }
  return o;
}
#define ADSB_FLEET_CAS(p, e, d) fleet_driver_cas((p), (e), (d))

#include "sim_support.h"

using namespace adsb;

namespace {
// the slots, and with ages the last_seen clocks beside them (never cleared: any bytes at first)
struct Store {
  Guarded<unsigned long long> keys, ann;
  Guarded<Plane> planes;
  Guarded<long long> seen;
  long long cap = 0;
  bool ages = false;
  void build(long long c, bool ages_) {
    cap = c; ages = ages_;
    keys.reset((size_t)c, 0xFF); ann.reset((size_t)c, 0xFF); planes.reset((size_t)c, 0);
    if (ages) seen.reset((size_t)c, 0xA5);
  }
  FleetStore view() { FleetStore v; v.keys = keys.p(); v.ann = ann.p(); v.planes = planes.p(); v.mask = (unsigned)(cap - 1); return v; }
  long long* seen_p() { return ages ? seen.p() : nullptr; }
  bool ok() const { return keys.ok() && ann.ok() && planes.ok() && seen.ok(); }
};

constexpr long long kMinCap = 256, kMaxCap = 1ll << 27;

struct Fleet {
  int fec = 0, all = 1;
  bool ages = false;
  double fs = 1.0;
  std::vector<double> start;
  std::vector<unsigned> gen;
  std::vector<long long> slots, planes;
  long long used = 0, live_slots = 0, live_planes = 0, grows = 0, max_cap = kMaxCap;
  unsigned long long call = 0;
  Store st;
};

Fleet* open_fleet(int n_streams, long long slots, int fec, int all, bool ages, double fs) {
  Fleet* F = new Fleet();
  F->fec = fec; F->all = all; F->ages = ages; F->fs = fs;
  F->start.assign((size_t)n_streams, 0.0); F->gen.assign((size_t)n_streams, 0u);
  F->slots.assign((size_t)n_streams, 0); F->planes.assign((size_t)n_streams, 0);
  long long cap = kMinCap;
  while (cap < slots) cap *= 2;
  F->st.build(cap, ages);
  return F;
}

// fleet_rehash: the live slots into a store of new_cap slots, with ages by k_ages_rehash, which moves last_seen with its slot;
// cutoffs ([n_streams]) make that an expiry, the dropped planes taken off the books.  0, or -1 (a guard), -3 (the kernel's
// error word, or counts that cannot be)
int rehash(Fleet& F, long long new_cap, int grid, bool renumber = false, const long long* cutoffs = nullptr, long long* n_removed = nullptr) {
  const size_t ns = F.gen.size();
  Store to;
  to.build(new_cap, F.ages);
  Guarded<long long> cut(ns, 0);
  Guarded<unsigned> gen(ns, 0);
  Guarded<FleetCount> removed(ns, 0);
  Guarded<int> err(1, 0);
  for (size_t s = 0; s < ns; ++s) gen.p()[s] = F.gen[s];
  for (size_t s = 0; cutoffs && s < ns; ++s) cut.p()[s] = cutoffs[s];
  if (F.ages) {
    FleetAges g{};
    g.from_seen = F.st.seen_p(); g.to_seen = to.seen_p();
    if (cutoffs) { g.cutoffs = cut.p(); g.removed = removed.p(); }
    hipsim::launch(k_ages_rehash, (unsigned)grid, (unsigned)kThreads, F.st.view(), to.view(), (const unsigned*)gen.p(), (int)ns,
                   renumber ? 1 : 0, err.p(), g);
  } else {
    hipsim::launch(k_fleet_rehash, (unsigned)grid, (unsigned)kThreads, F.st.view(), to.view(), (const unsigned*)gen.p(), (int)ns,
                   renumber ? 1 : 0, err.p());
  }
  if (!F.st.ok() || !to.ok() || !gen.ok() || !err.ok() || !cut.ok() || !removed.ok()) return -1;
  if (err.p()[0]) return -3;
  F.st = std::move(to);
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

int reset_stream(Fleet& F, size_t s) {
  F.live_slots -= F.slots[s]; F.live_planes -= F.planes[s];
  F.slots[s] = F.planes[s] = 0;
  if (F.gen[s] < kFleetGenMax) { ++F.gen[s]; return 0; }
  F.gen[s] = ~0u;
  const int r = rehash(F, F.st.cap, 3);
  F.gen[s] = 0;
  return r;
}

// the key of (stream, address 0) in the stream's current generation
unsigned long long key_base(const Fleet& F, size_t s) {
  return ((unsigned long long)F.gen[s] << (kFleetAddrBits + kFleetStreamBits)) | ((unsigned long long)s << kFleetAddrBits);
}

// The records' flags as the pipeline in front leaves them (k_dec_pdu_flags, k_fec_slices; b14: n PDUs, corrected in place),
// then 32-byte records with the offsets given.  dem (may be null): dem[t] == 0 is a record without ADSB_BURST_DEMOD.
// 0, or -1 (a guard)
int build_recs(Guarded<unsigned char>& b14, const long long* offset, const unsigned char* dem, int n, int fec, int grid, Guarded<Rec>& recs) {
  Guarded<unsigned char> ok((size_t)n, 0);
  hipsim::launch(k_dec_pdu_flags, (unsigned)grid, (unsigned)kThreads, (const unsigned char*)b14.p(), ok.p(), n);
  if (fec) hipsim::launch(k_fec_slices, (unsigned)grid, (unsigned)kThreads, b14.p(), ok.p(), n);
  if (!b14.ok() || !ok.ok()) return -1;
  recs.reset((size_t)n, 0);
  for (int t = 0; t < n; ++t) {
    const unsigned char* p = b14.p() + (size_t)t * 14;
    const unsigned o = ok.p()[t];
    unsigned long long w2 = 0, w3 = 0;
    for (int k = 0; k < 8; ++k) w2 |= (unsigned long long)p[k] << (8 * k);
    for (int k = 0; k < 6; ++k) w3 |= (unsigned long long)p[8 + k] << (8 * k);
    unsigned fl = (o & 0xE1u) | ((o & 6u) << 13);                      // (air_load's reading of an ok[] byte)
    if (dem && !dem[t]) fl = kKept;                                    // a record that publishes nothing
    Rec& r = recs.p()[t];
    r.w[0] = (unsigned long long)offset[t];
    r.w[1] = 0; r.w[2] = w2; r.w[3] = w3 | ((unsigned long long)fl << 48);
  }
  return 0;
}

// The decode step of one call's final list, as adsb_hip.hip's fleet_step runs it from the growth rule on: recs[n] in n_items
// items (items: n_items + 1 entries, the last the end mark), item k's counts booked under stream book[k].  ts_over: null, or
// n timestamps written over k_fleet_classify's (the shared decoder's true ones).  rows: n rows, in list positions.
// 0; -1: a kernel wrote behind one of its arrays; -2: a sorted key that names no record or no slot (the fold is not run);
// -3: a kernel set the error word, or the claims do not add up; -4: the store would exceed its largest size (refused: nothing
// has changed)
int decode_step(Fleet& F, Guarded<Rec>& recs, int n, Guarded<FleetItem>& items, int n_items, const int* book, const double* ts_over, int grid,
                Guarded<DecRow>& rows) {
  const bool renumber = F.call >= 0xFFFFFFFEull;
  if ((F.used + n) * 2 > F.st.cap || renumber) {
    const long long old_cap = F.st.cap;
    long long cap = old_cap;
    while ((F.live_slots + n) * 2 > cap) cap *= 2;
    if (cap > F.max_cap) return -4;
    const int r = rehash(F, cap, grid, renumber);
    if (r) return r;
    if (cap > old_cap) F.grows++;
  }
  Guarded<FleetCount> count((size_t)n_items, 0);
  Guarded<int> ncond((size_t)n_items + 1, 0), err(1, 0);
  KeyPair k((size_t)n);
  Guarded<double> tsd((size_t)n, 0xA5);
  rows.reset((size_t)n, 0xA5);
  FleetArgs a{};
  a.recs = recs.p(); a.n = n; a.n_items = n_items; a.items = items.p(); a.count = count.p(); a.ncond = ncond.p(); a.error = err.p();
  a.s = F.st.view(); a.call = F.call << 32; a.fec = F.fec; a.all = F.all; a.fs = F.fs;
  a.keys = k.keys.p(); a.sorted = k.sorted.p(); a.ts = tsd.p(); a.rows = rows.p(); a.seen = F.st.seen_p();
  auto guards = [&]() {
    return recs.ok() && items.ok() && count.ok() && ncond.ok() && err.ok() && k.ok() && tsd.ok() && rows.ok() && F.st.ok();
  };
  const long long claims0 = g_fleet_claims;
  hipsim::launch(k_fleet_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_fleet_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_fleet_cond, (unsigned)n_items, 64u, a);
  hipsim::launch(k_fleet_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  hipsim::launch(k_fleet_classify, (unsigned)grid, (unsigned)kThreads, a);
  if (!guards()) return -1;
  if (ts_over) memcpy(tsd.p(), ts_over, (size_t)n * sizeof(double));
  if (sort_keys(k.keys.p(), k.sorted.p(), n, 32, 60) || !guards()) return -1;
  for (int i = 0; i < n; ++i) {                                   // the fold reads the records and the slots these name
    const unsigned long long key = k.sorted.p()[i];
    if (key != kDecNoKey && ((unsigned)key >= (unsigned)n || (key >> 32) >= (unsigned long long)F.st.cap)) return -2;
  }
  hipsim::launch(k_fleet_fold, (unsigned)((n + kThreads - 1) / kThreads), (unsigned)kThreads, a);
  if (!guards()) return -1;
  if (err.p()[0]) return -3;
  long long claimed = 0;
  for (int i = 0; i < n_items; ++i) {
    const size_t s = (size_t)book[i];
    const FleetCount c = count.p()[i];
    F.slots[s] += c.slots; F.planes[s] += c.planes;
    F.live_slots += c.slots; F.live_planes += c.planes; F.used += c.slots;
    claimed += c.slots;
  }
  if (claimed != g_fleet_claims - claims0) return -3;            // every claim is counted by exactly one item
  F.call++;
  return 0;
}
}  // namespace

extern "C" {

int sim_fleet_slot_bytes() { return (int)(16 + sizeof(Plane)); }
int sim_fleet_row_bytes() { return (int)sizeof(DecRow); }
int sim_fleet_sort_tile() { return kSortTile; }
unsigned sim_fleet_gen_max() { return kFleetGenMax; }
long long sim_fleet_claims() { return g_fleet_claims; }

void* sim_fleet_open(int n_streams, long long slots, int fec, int all) { return open_fleet(n_streams, slots, fec, all, false, 1.0); }
void sim_fleet_close(void* h) { delete (Fleet*)h; }
void sim_fleet_set_start(void* h, int stream, double start) { ((Fleet*)h)->start[(size_t)stream] = start; }
// test hook: the generation of a stream that holds nothing (to reach the wrap without a million resets)
void sim_fleet_set_gen(void* h, int stream, unsigned gen) { ((Fleet*)h)->gen[(size_t)stream] = gen; }
// test hook: the number of the next call (to reach the renumbering without 2^32 calls)
void sim_fleet_set_call(void* h, unsigned long long call) { ((Fleet*)h)->call = call; }
unsigned long long sim_fleet_get_call(void* h) { return ((Fleet*)h)->call; }
int sim_fleet_reset(void* h, int stream) { return reset_stream(*(Fleet*)h, (size_t)stream); }
void sim_fleet_stats(void* h, long long* planes, long long* cap, long long* grows, long long* used) {
  const Fleet& F = *(Fleet*)h;
  *planes = F.live_planes; *cap = F.st.cap; *grows = F.grows; *used = F.used;
}
// the slots whose key is not empty (live and stale ones), counted in the store itself
long long sim_fleet_taken(void* h) {
  Fleet& F = *(Fleet*)h;
  long long k = 0;
  for (long long i = 0; i < F.st.cap; ++i) k += F.st.keys.p()[i] != kFleetEmpty;
  return k;
}

// One call: n PDUs (bits14: n x 14) with a timestamp and a stream index each, in any interleaving; a stream's PDUs keep
// their order.  The driver groups them into one item per stream that appears (items in order of first appearance), as a
// stream-batch call's final list holds them, and gives rows (n x 72 bytes) back in the caller's order.  The decoder's clock
// of a PDU is (long long)ts: a record's offset is that minus the whole seconds of its stream's start, at fs = 1.
// 0, or -1 .. -4 as decode_step; -5: a bad stream index.
int sim_fleet_call(void* h, const unsigned char* bits14, const double* ts, const int* stream, int n, int grid, void* rows_out) {
  Fleet& F = *(Fleet*)h;
  if (n <= 0) return 0;
  for (int i = 0; i < n; ++i) if (stream[i] < 0 || (size_t)stream[i] >= F.gen.size()) return -5;
  // the final list: items of contiguous records
  std::vector<int> order_of_stream(F.gen.size(), -1), item_stream;
  for (int i = 0; i < n; ++i)
    if (order_of_stream[(size_t)stream[i]] < 0) { order_of_stream[(size_t)stream[i]] = (int)item_stream.size(); item_stream.push_back(stream[i]); }
  const int n_items = (int)item_stream.size();
  std::vector<std::vector<int>> members((size_t)n_items);
  for (int i = 0; i < n; ++i) members[(size_t)order_of_stream[(size_t)stream[i]]].push_back(i);
  std::vector<int> src;                         // list position -> caller's index
  Guarded<FleetItem> items((size_t)n_items + 1, 0);
  for (int k = 0; k < n_items; ++k) {
    const size_t s = (size_t)item_stream[(size_t)k];
    FleetItem& it = items.p()[k];
    it.first = (int)src.size(); it.stream = (int)s; it.base = key_base(F, s);
    it.start = (double)(long long)F.start[s];
    src.insert(src.end(), members[(size_t)k].begin(), members[(size_t)k].end());
  }
  items.p()[n_items].first = n; items.p()[n_items].stream = -1;
  Guarded<unsigned char> b14((size_t)n * 14, 0);
  std::vector<long long> offset((size_t)n);
  for (int t = 0; t < n; ++t) {
    const size_t i = (size_t)src[(size_t)t];
    memcpy(b14.p() + (size_t)t * 14, bits14 + i * 14, 14);
    offset[(size_t)t] = (long long)ts[i] - (long long)F.start[(size_t)stream[i]];
  }
  Guarded<Rec> recs;
  Guarded<DecRow> rows;
  int r;
  if ((r = build_recs(b14, offset.data(), nullptr, n, F.fec, grid, recs)) ||
      (r = decode_step(F, recs, n, items, n_items, item_stream.data(), nullptr, grid, rows)))
    return r;
  for (int t = 0; t < n; ++t) memcpy((char*)rows_out + (size_t)src[(size_t)t] * sizeof(DecRow), &rows.p()[t], sizeof(DecRow));
  return 0;
}
}
