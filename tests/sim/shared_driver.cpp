// shared_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the shared decoder of a fleet (ADSB_FLAG_STREAM_DECODE_SHARED) on the
// SIMT emulator in hipsim.h, on host memory: the time order's kernels of gr_adsb_amd/csrc/adsb_shared_device.h (k_shared_keys,
// k_shared_sort_*, k_shared_gather, k_shared_scatter) around the per-stream decoders' kernels of adsb_device.h (k_fleet_*,
// k_dec_sort_*, k_ages_rehash), in the order adsb_hip.hip's fleet_step queues them on a shared context, with the host's growth
// rule in front and its bookkeeping (everything under stream index 0) behind -- RESTATED here, not shared, as
// fleet_driver.cpp does: the host's own code runs only in tests/test_gpu_shared_decode.py.
// Never linked into libadsb_hip.so.
#include "hipsim.h"

#include <algorithm>
#include <vector>

inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, sizeof r); return r; }

#include "../../gr_adsb_amd/csrc/adsb_device.h"
#include "../../gr_adsb_amd/csrc/adsb_shared_device.h"

using namespace adsb;
namespace sh = adsb_shared;

static_assert(sizeof(Rec) == sh::kRecWords * 8 && sizeof(DecRow) == sh::kRowWords * 8, "the sizes adsb_shared_device.h assumes");

namespace {
constexpr unsigned char kGuardByte = 0xA5;
constexpr size_t kGuardBytes = 256;

// n elements a kernel may touch and guard bytes behind them
template <class T>
struct Guarded {
  std::vector<unsigned char> raw;
  size_t n = 0;
  Guarded() = default;
  Guarded(size_t n_, int fill) { reset(n_, fill); }
  void reset(size_t n_, int fill) {
    n = n_;
    raw.assign(n * sizeof(T) + kGuardBytes, kGuardByte);
    std::fill(raw.begin(), raw.begin() + (long)(n * sizeof(T)), (unsigned char)fill);
  }
  T* p() { return reinterpret_cast<T*>(raw.data()); }
  bool ok() const {
    for (size_t k = n * sizeof(T); k < raw.size(); ++k) if (raw[k] != kGuardByte) return false;
    return true;
  }
};

struct Store {
  Guarded<unsigned long long> keys, ann;
  Guarded<Plane> planes;
  Guarded<long long> seen;
  long long cap = 0;
  void build(long long c) {
    cap = c;
    keys.reset((size_t)c, 0xFF); ann.reset((size_t)c, 0xFF); planes.reset((size_t)c, 0); seen.reset((size_t)c, 0);
  }
  FleetStore view() { FleetStore v; v.keys = keys.p(); v.ann = ann.p(); v.planes = planes.p(); v.mask = (unsigned)(cap - 1); return v; }
  bool ok() const { return keys.ok() && ann.ok() && planes.ok() && seen.ok(); }
};

constexpr long long kMinCap = 256;

struct Shared {
  int fec = 0, all = 1, ages = 0;
  double fs = 1.0;
  std::vector<double> start;
  std::vector<unsigned> gen;                      // only gen[0] is ever in a key
  long long slots = 0, planes = 0;                // stream 0's books: the decoder's
  long long used = 0, grows = 0, max_cap = 1ll << 27;
  unsigned long long call = 0;
  Store st;
};

// fleet_rehash: the live slots into a store of new_cap slots; cutoff: adsb_stream_planes_expire's, for stream 0
int rehash(Shared& F, long long new_cap, int grid, const long long* cutoff = nullptr, long long* n_removed = nullptr) {
  Store to;
  to.build(new_cap);
  const size_t ns = F.gen.size();
  Guarded<unsigned> gen(ns, 0);
  for (size_t s = 0; s < ns; ++s) gen.p()[s] = F.gen[s];
  Guarded<int> err(1, 0);
  Guarded<long long> cut(ns, 0);
  Guarded<FleetCount> removed(ns, 0);
  if (F.ages) {
    FleetAges g{};
    g.from_seen = F.st.seen.p(); g.to_seen = to.seen.p();
    if (cutoff) {
      for (size_t s = 0; s < ns; ++s) cut.p()[s] = *cutoff;
      g.cutoffs = cut.p(); g.removed = removed.p();
    }
    hipsim::launch(k_ages_rehash, (unsigned)grid, (unsigned)kThreads, F.st.view(), to.view(), (const unsigned*)gen.p(), (int)ns, 0, err.p(), g);
  } else {
    hipsim::launch(k_fleet_rehash, (unsigned)grid, (unsigned)kThreads, F.st.view(), to.view(), (const unsigned*)gen.p(), (int)ns, 0, err.p());
  }
  if (!F.st.ok() || !to.ok() || !gen.ok() || !err.ok() || !cut.ok() || !removed.ok()) return -1;
  if (err.p()[0]) return -3;
  F.st = std::move(to);
  for (size_t s = 0; s < ns; ++s) {
    if (s != 0 && (removed.p()[s].slots || removed.p()[s].planes)) return -3;     // nobody but stream 0 holds anything
    F.slots -= removed.p()[s].slots; F.planes -= removed.p()[s].planes;
  }
  if (n_removed) *n_removed = removed.p()[0].planes;
  F.used = F.slots;
  return 0;
}

// the stable pair sort alone: keys / vals [n] hold the result.  0, or -1 (a guard)
int sort_pairs(Guarded<unsigned long long>& keys, Guarded<unsigned>& vals, int n) {
  Guarded<unsigned long long> keys_tmp((size_t)n, 0xA5);
  Guarded<unsigned> vals_tmp((size_t)n, 0xA5);
  const int nblk = (n + sh::kSortTile - 1) / sh::kSortTile;
  Guarded<unsigned> hist((size_t)nblk * sh::kDigits, 0xA5);
  unsigned long long *ki = keys.p(), *ko = keys_tmp.p();
  unsigned *vi = vals.p(), *vo = vals_tmp.p();
  for (int shift = 0; shift < 64; shift += sh::kDigitBits) {
    hipsim::launch(sh::k_shared_sort_hist, (unsigned)nblk, (unsigned)sh::kThreads, (const unsigned long long*)ki, n, shift, hist.p());
    hipsim::launch(sh::k_shared_sort_scan, 1u, (unsigned)sh::kThreads, hist.p(), nblk * sh::kDigits);
    hipsim::launch(sh::k_shared_sort_scatter, (unsigned)nblk, (unsigned)sh::kThreads, (const unsigned long long*)ki, (const unsigned*)vi, ko, vo,
                   n, shift, (const unsigned*)hist.p());
    std::swap(ki, ko); std::swap(vi, vo);
    if (!keys.ok() || !vals.ok() || !keys_tmp.ok() || !vals_tmp.ok() || !hist.ok()) return -1;
  }
  return 0;
}
}  // namespace

extern "C" {

int sim_shared_row_bytes() { return (int)sizeof(DecRow); }
int sim_shared_sort_tile() { return sh::kSortTile; }

// The order alone: n timestamps, given as doubles -> their keys (time_key, the map k_shared_keys uses) through the stable
// pair sort.  order_out[n]: the sorted values, keys_out[n]: the sorted keys.  vals0: null (the values are 0 .. n-1) or the
// values to carry.  0, or -1 (a guard byte overwritten).
int sim_shared_sort(const double* ts, const unsigned* vals0, int n, unsigned* order_out, unsigned long long* keys_out) {
  if (n <= 0) return 0;
  Guarded<unsigned long long> keys((size_t)n, 0);
  Guarded<unsigned> vals((size_t)n, 0);
  for (int i = 0; i < n; ++i) { keys.p()[i] = sh::time_key(ts[i]); vals.p()[i] = vals0 ? vals0[i] : (unsigned)i; }
  const int r = sort_pairs(keys, vals, n);
  if (r) return r;
  memcpy(order_out, vals.p(), (size_t)n * sizeof(unsigned));
  memcpy(keys_out, keys.p(), (size_t)n * sizeof(unsigned long long));
  return 0;
}
// raw 64-bit keys instead of doubles (keys that differ in one byte only)
int sim_shared_sort_keys(const unsigned long long* keys0, int n, unsigned* order_out) {
  if (n <= 0) return 0;
  Guarded<unsigned long long> keys((size_t)n, 0);
  Guarded<unsigned> vals((size_t)n, 0);
  for (int i = 0; i < n; ++i) { keys.p()[i] = keys0[i]; vals.p()[i] = (unsigned)i; }
  const int r = sort_pairs(keys, vals, n);
  if (r) return r;
  for (int i = 1; i < n; ++i) if (keys.p()[i - 1] > keys.p()[i]) return -2;
  memcpy(order_out, vals.p(), (size_t)n * sizeof(unsigned));
  return 0;
}

void* sim_shared_open(int n_streams, long long slots, int fec, int all, int ages, double fs) {
  Shared* F = new Shared();
  F->fec = fec; F->all = all; F->ages = ages; F->fs = fs;
  F->start.assign((size_t)n_streams, 0.0); F->gen.assign((size_t)n_streams, 0u);
  long long cap = kMinCap;
  while (cap < slots) cap *= 2;
  F->st.build(cap);
  return F;
}
void sim_shared_close(void* h) { delete (Shared*)h; }
void sim_shared_set_start(void* h, int stream, double start) { ((Shared*)h)->start[(size_t)stream] = start; }
void sim_shared_set_max_cap(void* h, long long cap) { ((Shared*)h)->max_cap = cap; }
// adsb_streams_decoder_reset: a new generation of index 0
void sim_shared_reset(void* h) {
  Shared& F = *(Shared*)h;
  F.slots = F.planes = 0;
  ++F.gen[0];
}
void sim_shared_stats(void* h, long long* planes, long long* cap, long long* grows, long long* used) {
  const Shared& F = *(Shared*)h;
  *planes = F.planes; *cap = F.st.cap; *grows = F.grows; *used = F.used;
}
// a digest of the whole state: the store's arrays byte for byte, in slot order, and the books
unsigned long long sim_shared_digest(void* h) {
  Shared& F = *(Shared*)h;
  unsigned long long d = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { d ^= ((const unsigned char*)p)[i]; d *= 1099511628211ull; } };
  mix(F.st.keys.p(), (size_t)F.st.cap * 8); mix(F.st.ann.p(), (size_t)F.st.cap * 8);
  mix(F.st.planes.p(), (size_t)F.st.cap * sizeof(Plane)); mix(F.st.seen.p(), (size_t)F.st.cap * 8);
  const long long books[6] = {F.slots, F.planes, F.used, F.grows, (long long)F.call, (long long)F.gen[0]};
  mix(books, sizeof books);
  return d;
}
// the decoder's planes read from the store itself: addresses and last_seen clocks (cap entries at the most) -> their number
int sim_shared_planes(void* h, int* addr, long long* seen, int cap) {
  Shared& F = *(Shared*)h;
  int k = 0;
  for (long long i = 0; i < F.st.cap; ++i) {
    const unsigned long long key = F.st.keys.p()[i];
    if (key == kFleetEmpty || (key >> kFleetAddrBits) != ((unsigned long long)F.gen[0] << kFleetStreamBits)) continue;
    if (!(F.st.planes.p()[i].present & kHasPlane)) continue;
    if (k < cap) { addr[k] = (int)(key & 0xFFFFFFu); seen[k] = F.st.seen.p()[i]; }
    ++k;
  }
  return k;
}
// adsb_stream_planes_expire for the one decoder: its planes with last_seen < cutoff are dropped by a rehash
long long sim_shared_expire(void* h, long long cutoff, int grid) {
  Shared& F = *(Shared*)h;
  long long removed = 0;
  const int r = rehash(F, F.st.cap, grid, &cutoff, &removed);
  return r ? (long long)r : removed;
}

// One call.  The final list as a stream-batch call holds it: n records in n_items items (item i: stream item_stream[i],
// records [item_first[i], item_first[i + 1])), a record's PDU bits14[t] (14 bytes) and its offset.  dem[t] == 0: a record
// without ADSB_BURST_DEMOD.  Out, all in LIST positions: flags_out[n] (the records' 16 flag bits), rows_out (n x 72 bytes),
// ts_out[n]; order_out[n]: the publication order.
// 0; -1: a kernel wrote behind one of its arrays; -2: a sorted key that names no record or no slot, or an order that is no
// permutation; -3: a kernel set the error word, or the books do not add up; -4: the store would exceed its largest size (the
// call is refused: nothing has changed); -5: a bad argument.
int sim_shared_call(void* h, const unsigned char* bits14, const long long* offset, const unsigned char* dem, int n, const int* item_stream,
                    const int* item_first, int n_items, int grid, unsigned short* flags_out, void* rows_out, int* order_out, double* ts_out) {
  Shared& F = *(Shared*)h;
  if (n <= 0) return 0;
  if (n_items <= 0 || item_first[n_items] != n) return -5;
  for (int i = 0; i < n_items; ++i)
    if (item_stream[i] < 0 || (size_t)item_stream[i] >= F.gen.size() || item_first[i] > item_first[i + 1]) return -5;
  // the records' flags as the pipeline in front leaves them (k_dec_pdu_flags, k_fec_slices), then 32-byte records
  Guarded<unsigned char> b14((size_t)n * 14, 0), ok((size_t)n, 0);
  memcpy(b14.p(), bits14, (size_t)n * 14);
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
    unsigned fl = (o & 0xE1u) | ((o & 6u) << 13);                      // (air_load's reading of an ok[] byte)
    if (dem && !dem[t]) fl = kKept;                                    // a record that publishes nothing
    Rec& r = recs.p()[t];
    r.w[0] = (unsigned long long)offset[t];
    r.w[1] = 0; r.w[2] = w2; r.w[3] = w3 | ((unsigned long long)fl << 48);
  }
  // the host's growth rule (adsb_hip.hip fleet_step), before any kernel that touches the store
  if ((F.used + n) * 2 > F.st.cap) {
    const long long old_cap = F.st.cap;
    long long cap = old_cap;
    while ((F.slots + n) * 2 > cap) cap *= 2;
    if (cap > F.max_cap) return -4;
    const int r = rehash(F, cap, grid);
    if (r) return r;
    if (cap > old_cap) F.grows++;
  }
  // the time order
  Guarded<int> first((size_t)n_items + 1, 0);
  Guarded<double> start((size_t)n_items, 0);
  for (int i = 0; i <= n_items; ++i) first.p()[i] = item_first[i];
  for (int i = 0; i < n_items; ++i) start.p()[i] = F.start[(size_t)item_stream[i]];
  Guarded<unsigned long long> skeys((size_t)n, 0xA5);
  Guarded<unsigned> vals((size_t)n, 0xA5);
  Guarded<double> ts((size_t)n, 0xA5), ts_sorted((size_t)n, 0xA5);
  Guarded<Rec> srecs((size_t)n, 0xA5);
  Guarded<DecRow> srows((size_t)n, 0xA5), rows((size_t)n, 0xA5);
  Guarded<int> order((size_t)n, 0xA5);
  hipsim::launch(sh::k_shared_keys, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)recs.p(), n, (const int*)first.p(),
                 (const double*)start.p(), n_items, F.fs, skeys.p(), vals.p(), ts.p());
  if (!skeys.ok() || !vals.ok() || !ts.ok() || !recs.ok() || !first.ok() || !start.ok()) return -1;
  { const int r = sort_pairs(skeys, vals, n); if (r) return r; }
  hipsim::launch(sh::k_shared_gather, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)recs.p(), (const double*)ts.p(),
                 (const unsigned*)vals.p(), n, (unsigned long long*)srecs.p(), ts_sorted.p(), order.p());
  if (!srecs.ok() || !ts_sorted.ok() || !order.ok() || !recs.ok()) return -1;
  {
    std::vector<char> hit((size_t)n, 0);
    for (int r = 0; r < n; ++r) {
      const int t = order.p()[r];
      if (t < 0 || t >= n || hit[(size_t)t]) return -2;
      hit[(size_t)t] = 1;
    }
  }
  // the decode step on the time-ordered list: one item of stream 0
  Guarded<FleetItem> items(2, 0);
  items.p()[0].first = 0; items.p()[0].stream = 0; items.p()[0].start = 0;
  items.p()[0].base = (unsigned long long)F.gen[0] << (kFleetAddrBits + kFleetStreamBits);
  items.p()[1].first = n; items.p()[1].stream = -1;
  Guarded<FleetCount> count(1, 0);
  Guarded<int> ncond(2, 0), err(1, 0);
  Guarded<unsigned long long> keys((size_t)n + kSortTile, 0xA5), sorted((size_t)n + kSortTile, 0xA5);
  Guarded<double> tsd((size_t)n, 0xA5);
  FleetArgs a{};
  a.recs = srecs.p(); a.n = n; a.n_items = 1; a.items = items.p(); a.count = count.p(); a.ncond = ncond.p(); a.error = err.p();
  a.s = F.st.view(); a.call = F.call << 32; a.fec = F.fec; a.all = F.all; a.fs = F.fs;
  a.keys = keys.p(); a.sorted = sorted.p(); a.ts = tsd.p(); a.rows = srows.p(); a.seen = F.ages ? F.st.seen.p() : nullptr;
  auto guards = [&]() {
    return srecs.ok() && items.ok() && count.ok() && ncond.ok() && err.ok() && keys.ok() && sorted.ok() && tsd.ok() && srows.ok() && F.st.ok();
  };
  hipsim::launch(k_fleet_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_fleet_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_fleet_cond, 1u, 64u, a);
  hipsim::launch(k_fleet_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  hipsim::launch(k_fleet_classify, (unsigned)grid, (unsigned)kThreads, a);
  if (!guards()) return -1;
  memcpy(tsd.p(), ts_sorted.p(), (size_t)n * sizeof(double));           // the true timestamps over the one item's
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
      std::swap(in, out);
    }
    if (!hist.ok() || !guards()) return -1;
  }
  for (int i = 0; i < n; ++i) {                                   // the fold reads the records and the slots these name
    const unsigned long long k = sorted.p()[i];
    if (k != kDecNoKey && ((unsigned)k >= (unsigned)n || (k >> 32) >= (unsigned long long)F.st.cap)) return -2;
  }
  hipsim::launch(k_fleet_fold, (unsigned)((n + kThreads - 1) / kThreads), (unsigned)kThreads, a);
  if (!guards()) return -1;
  if (err.p()[0]) return -3;
  hipsim::launch(sh::k_shared_scatter, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)srecs.p(),
                 (const unsigned long long*)srows.p(), (const int*)order.p(), n, (unsigned long long*)recs.p(), (unsigned long long*)rows.p());
  if (!guards() || !recs.ok() || !rows.ok() || !order.ok()) return -1;
  const FleetCount c = count.p()[0];
  F.slots += c.slots; F.planes += c.planes; F.used += c.slots;
  F.call++;
  for (int t = 0; t < n; ++t) flags_out[t] = (unsigned short)(recs.p()[t].w[3] >> 48);
  memcpy(rows_out, rows.p(), (size_t)n * sizeof(DecRow));
  memcpy(order_out, order.p(), (size_t)n * sizeof(int));
  memcpy(ts_out, ts.p(), (size_t)n * sizeof(double));
  return 0;
}
}
