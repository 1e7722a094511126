// dedup_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs a shared decoder with ADSB_FLAG_STREAM_DEDUP on the SIMT emulator in
// hipsim.h, on host memory: the kernels of gr_adsb_amd/csrc/adsb_dedup_device.h (k_dedup_entries, k_dedup_find, k_dedup_merge,
// k_dedup_mark) inside shared_driver.cpp's call (the time order's kernels around fleet_driver.cpp's decode step), in the order
// adsb_hip.hip's fleet_step queues them, with the host's rule for the carry restated: a call merges into a second buffer, and
// the cut, hi and that buffer are taken only when the call is delivered.  Guarded buffers throughout.  The host's own code
// runs only in tests/test_gpu_dedup.py.  Never linked into libadsb_hip.so.
#include "shared_driver.cpp"

inline double __longlong_as_double(long long v) { double r; memcpy(&r, &v, sizeof r); return r; }

#include "../../gr_adsb_amd/csrc/adsb_dedup_device.h"

namespace dd = adsb_dedup;

static_assert(sizeof(Rec) == dd::kRecWords * 8 && sizeof(DecRow) == dd::kRowWords * 8, "the sizes adsb_dedup_device.h assumes");
static_assert(kDemod == 1u && kLongFmt == 64u, "the record flags adsb_dedup_device.h reads in word 3");

namespace {
struct Dedup {
  Fleet* F = nullptr;
  double window = 0.002, horizon = 1.0, hi = 0;
  std::vector<unsigned long long> carry;        // cnt entries of four words (the cut's prefix already dropped)
  long long duplicates = 0;
  void fresh() { carry.clear(); hi = 0; duplicates = 0; }
};
}  // namespace

extern "C" {

int sim_dedup_tile() { return dd::kTile; }
int sim_dedup_lds_bytes() { return dd::kLdsBytes; }

void* sim_dedup_open(int n_streams, long long slots, int fec, int all, int ages, double fs, double window, double horizon) {
  Dedup* D = new Dedup();
  D->F = open_fleet(n_streams, slots, fec, all, ages != 0, fs);
  D->window = window; D->horizon = horizon;
  return D;
}
void sim_dedup_close(void* h) { delete ((Dedup*)h)->F; delete (Dedup*)h; }
// the shared decoder behind it, for shared_driver.cpp's sim_shared_* calls (set_start, stats, digest, planes, expire)
void* sim_dedup_fleet(void* h) { return ((Dedup*)h)->F; }
// adsb_streams_decoder_reset: a fresh decoder, an empty carry
void sim_dedup_reset(void* h) { (void)reset_stream(*((Dedup*)h)->F, 0); ((Dedup*)h)->fresh(); }
// adsb_stream_reset on a shared context: the stream's framing state only (which this driver does not hold) -- adsb_hip.hip
// calls fleet_reset_stream, and with it the carry's fresh(), only where the context is NOT shared
void sim_dedup_stream_reset(void* h, int stream) { (void)h; (void)stream; }
void sim_dedup_stats(void* h, long long* duplicates, long long* carried, double* hi) {
  const Dedup& D = *(Dedup*)h;
  *duplicates = D.duplicates; *carried = (long long)(D.carry.size() / dd::kEntWords); *hi = D.hi;
}
// the carry's entries, in its order: ts, stream, marker (0: takes no part, 1: 56 bits, 2: 112 bits) -> their number
int sim_dedup_carry(void* h, double* ts, int* stream, int* marker, int cap) {
  const Dedup& D = *(Dedup*)h;
  const int n = (int)(D.carry.size() / dd::kEntWords);
  for (int i = 0; i < n && i < cap; ++i) {
    const unsigned long long* e = &D.carry[(size_t)i * dd::kEntWords];
    memcpy(&ts[i], &e[0], 8);
    stream[i] = (int)((e[3] >> 32) & 0xFFFFFFu); marker[i] = (int)(e[3] >> 56);
  }
  return n;
}
unsigned long long sim_dedup_digest(void* h) {
  const Dedup& D = *(Dedup*)h;
  unsigned long long d = sim_shared_digest(D.F);
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { d ^= ((const unsigned char*)p)[i]; d *= 1099511628211ull; } };
  mix(D.carry.data(), D.carry.size() * 8); mix(&D.hi, 8); mix(&D.duplicates, 8);
  return d;
}

// One call, as sim_shared_call; dup_out[n] at list positions.  The same return codes; -6: the cut k_dedup_merge states does
// not add up.
int sim_dedup_call(void* h, const unsigned char* bits14, const long long* offset, const unsigned char* dem, int n, const int* item_stream,
                   const int* item_first, int n_items, int grid, unsigned short* flags_out, void* rows_out, int* order_out, double* ts_out,
                   int* dup_out) {
  Dedup& D = *(Dedup*)h;
  Fleet& F = *D.F;
  if (n <= 0) return 0;
  if (n_items <= 0 || item_first[n_items] != n) return -5;
  for (int i = 0; i < n_items; ++i)
    if (item_stream[i] < 0 || (size_t)item_stream[i] >= F.gen.size() || item_first[i] > item_first[i + 1]) return -5;
  Guarded<unsigned char> b14((size_t)n * 14, 0);
  memcpy(b14.p(), bits14, (size_t)n * 14);
  Guarded<Rec> recs;
  int r;
  if ((r = build_recs(b14, offset, dem, n, F.fec, grid, recs))) return r;
  Guarded<int> first((size_t)n_items + 1, 0), streams((size_t)n_items, 0);
  Guarded<double> start((size_t)n_items, 0);
  for (int i = 0; i <= n_items; ++i) first.p()[i] = item_first[i];
  for (int i = 0; i < n_items; ++i) { start.p()[i] = F.start[(size_t)item_stream[i]]; streams.p()[i] = item_stream[i]; }
  Guarded<unsigned long long> skeys((size_t)n, 0xA5);
  Guarded<unsigned> vals((size_t)n, 0xA5);
  Guarded<double> ts((size_t)n, 0xA5), ts_sorted((size_t)n, 0xA5);
  Guarded<Rec> srecs((size_t)n, 0xA5);
  Guarded<DecRow> srows, rows((size_t)n, 0xA5);
  Guarded<int> order((size_t)n, 0xA5);
  hipsim::launch(sh::k_shared_keys, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)recs.p(), n, (const int*)first.p(),
                 (const double*)start.p(), n_items, F.fs, skeys.p(), vals.p(), ts.p());
  if (!skeys.ok() || !vals.ok() || !ts.ok() || !recs.ok() || !first.ok() || !start.ok()) return -1;
  if ((r = sort_pairs(skeys, vals, n))) return r;
  hipsim::launch(sh::k_shared_gather, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)recs.p(), (const double*)ts.p(),
                 (const unsigned*)vals.p(), n, (unsigned long long*)srecs.p(), ts_sorted.p(), order.p());
  if (!srecs.ok() || !ts_sorted.ok() || !order.ok() || !recs.ok()) return -1;
  {
    std::vector<char> hit((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
      const int t = order.p()[k];
      if (t < 0 || t >= n || hit[(size_t)t]) return -2;
      hit[(size_t)t] = 1;
    }
  }
  // the de-duplication step: entries, verdicts (duplicates lose kDemod in srecs), the merge into the carry's other buffer
  const int nc = (int)(D.carry.size() / dd::kEntWords);
  Guarded<unsigned long long> ent((size_t)n * dd::kEntWords, 0xA5), carry((size_t)nc * dd::kEntWords, 0),
      merged((size_t)(nc + n) * dd::kEntWords, 0xA5);
  if (nc) memcpy(carry.p(), D.carry.data(), D.carry.size() * 8);
  Guarded<int> dup((size_t)n, 0xA5);
  Guarded<dd::State> state(1, 0);
  hipsim::launch(dd::k_dedup_entries, (unsigned)grid, (unsigned)dd::kThreads, (const unsigned long long*)srecs.p(), (const double*)ts_sorted.p(),
                 (const int*)order.p(), n, (const int*)first.p(), (const int*)streams.p(), n_items, ent.p());
  if (!ent.ok() || !srecs.ok() || !streams.ok()) return -1;
  hipsim::launch(dd::k_dedup_find, (unsigned)grid, (unsigned)dd::kThreads, (const unsigned long long*)ent.p(), n,
                 (const unsigned long long*)carry.p(), nc, D.window, (const int*)order.p(), (unsigned long long*)srecs.p(), dup.p());
  if (!ent.ok() || !carry.ok() || !srecs.ok() || !dup.ok() || !order.ok()) return -1;
  hipsim::launch(dd::k_dedup_merge, (unsigned)grid, (unsigned)dd::kThreads, (const unsigned long long*)carry.p(), nc,
                 (const unsigned long long*)ent.p(), n, D.horizon, merged.p(), state.p());
  if (!ent.ok() || !carry.ok() || !merged.ok() || !state.ok()) return -1;
  if (nc && memcmp(carry.p(), D.carry.data(), D.carry.size() * 8) != 0) return -6;      // the carry itself is read-only
  // the decode step on the time-ordered list: one item of stream 0, the true timestamps over the one item's
  Guarded<FleetItem> items(2, 0);
  items.p()[0].base = key_base(F, 0);
  items.p()[1].first = n; items.p()[1].stream = -1;
  const int book = 0;
  if ((r = decode_step(F, srecs, n, items, 1, &book, ts_sorted.p(), grid, srows))) return r;
  hipsim::launch(sh::k_shared_scatter, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)srecs.p(),
                 (const unsigned long long*)srows.p(), (const int*)order.p(), n, (unsigned long long*)recs.p(), (unsigned long long*)rows.p());
  if (!srecs.ok() || !srows.ok() || !recs.ok() || !rows.ok() || !order.ok()) return -1;
  hipsim::launch(dd::k_dedup_mark, (unsigned)grid, (unsigned)dd::kThreads, (const int*)dup.p(), n, (unsigned long long*)recs.p(),
                 (unsigned long long*)rows.p());
  if (!recs.ok() || !rows.ok() || !dup.ok()) return -1;
  // delivered: the cut, hi and the merged buffer are taken
  const dd::State s = state.p()[0];
  if (s.off < 0 || s.cnt < 1 || s.off + s.cnt != nc + n) return -6;
  for (int i = 1; i < nc + n; ++i)
    if (dd::ent_key(merged.p(), i - 1) > dd::ent_key(merged.p(), i)) return -6;
  D.carry.assign(merged.p() + (size_t)s.off * dd::kEntWords, merged.p() + (size_t)(s.off + s.cnt) * dd::kEntWords);
  D.hi = s.hi;
  for (int t = 0; t < n; ++t) D.duplicates += dup.p()[t] != dd::kDupNone;
  for (int t = 0; t < n; ++t) flags_out[t] = (unsigned short)(recs.p()[t].w[3] >> 48);
  memcpy(rows_out, rows.p(), (size_t)n * sizeof(DecRow));
  memcpy(order_out, order.p(), (size_t)n * sizeof(int));
  memcpy(ts_out, ts.p(), (size_t)n * sizeof(double));
  memcpy(dup_out, dup.p(), (size_t)n * sizeof(int));
  return 0;
}

// The four k_dedup_* kernels ALONE, in fleet_step's order, on stated arrays (tests/gpu/dedup_device_driver.hip is this entry on
// the device).  In: the call's records in time order sorted_recs[n][4] with sorted_ts[n] and order[n] (a permutation: place ->
// list position), first[n_items + 1] and item_stream[n_items]; the carry's words carry[nc][4]; recs[n][4] / rows[n][9]: the
// delivered records and rows k_dedup_mark works on, at list positions.  Out: ent_out[n][4] (k_dedup_entries), dup_out[n] and
// sorted_out[n][4] (the time-ordered records behind k_dedup_find), merged_out[nc + n][4] and state_out (a State, 16 bytes:
// k_dedup_merge), recs_out[n][4] and rows_out[n][9] (k_dedup_mark).  n == 0: nothing is run, as in the call.
// 0; -1: a guard byte, or a byte of order[], first[] or item_stream[], was overwritten; -5: a bad argument; -6: the carry was
// written to, or the cut k_dedup_merge states does not add up.
int sim_dedup_step(const unsigned long long* sorted_recs, const double* sorted_ts, const int* order, int n, const int* first,
                   const int* item_stream, int n_items, const unsigned long long* carry_in, int nc, double window, double horizon, int grid,
                   const unsigned long long* recs_in, const unsigned long long* rows_in, unsigned long long* ent_out, int* dup_out,
                   unsigned long long* sorted_out, unsigned long long* merged_out, void* state_out, unsigned long long* recs_out,
                   unsigned long long* rows_out) {
  if (n < 0 || nc < 0 || grid < 1) return -5;
  if (n == 0) return 0;
  if (n_items <= 0 || first[0] != 0 || first[n_items] != n || !(window >= 0) || !(horizon >= 0)) return -5;
  for (int i = 0; i < n_items; ++i)
    if (first[i] > first[i + 1]) return -5;
  {
    std::vector<char> hit((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
      const int t = order[k];
      if (t < 0 || t >= n || hit[(size_t)t]) return -5;
      hit[(size_t)t] = 1;
    }
  }
  const size_t rw = dd::kRecWords, ew = dd::kEntWords, ww = dd::kRowWords;
  Guarded<unsigned long long> srecs((size_t)n * rw, 0), carry((size_t)nc * ew, 0), ent((size_t)n * ew, 0xA5), merged((size_t)(nc + n) * ew, 0xA5),
      recs((size_t)n * rw, 0), rows((size_t)n * ww, 0);
  Guarded<double> sts((size_t)n, 0);
  Guarded<int> ord((size_t)n, 0), fst((size_t)n_items + 1, 0), streams((size_t)n_items, 0), dup((size_t)n, 0xA5);
  Guarded<dd::State> state(1, 0xA5);
  memcpy(srecs.p(), sorted_recs, (size_t)n * rw * 8);
  memcpy(sts.p(), sorted_ts, (size_t)n * 8);
  memcpy(ord.p(), order, (size_t)n * 4);
  memcpy(fst.p(), first, ((size_t)n_items + 1) * 4);
  memcpy(streams.p(), item_stream, (size_t)n_items * 4);
  if (nc) memcpy(carry.p(), carry_in, (size_t)nc * ew * 8);
  memcpy(recs.p(), recs_in, (size_t)n * rw * 8);
  memcpy(rows.p(), rows_in, (size_t)n * ww * 8);
  const auto all_ok = [&] {
    return srecs.ok() && carry.ok() && ent.ok() && merged.ok() && recs.ok() && rows.ok() && sts.ok() && ord.ok() && fst.ok() && streams.ok() &&
           dup.ok() && state.ok() && memcmp(ord.p(), order, (size_t)n * 4) == 0 && memcmp(fst.p(), first, ((size_t)n_items + 1) * 4) == 0 &&
           memcmp(streams.p(), item_stream, (size_t)n_items * 4) == 0;
  };
  const auto carry_same = [&] { return nc == 0 || memcmp(carry.p(), carry_in, (size_t)nc * ew * 8) == 0; };

  hipsim::launch(dd::k_dedup_entries, (unsigned)grid, (unsigned)dd::kThreads, (const unsigned long long*)srecs.p(), (const double*)sts.p(),
                 (const int*)ord.p(), n, (const int*)fst.p(), (const int*)streams.p(), n_items, ent.p());
  if (!all_ok()) return -1;
  if (memcmp(srecs.p(), sorted_recs, (size_t)n * rw * 8) != 0) return -1;      // k_dedup_entries only reads the records
  memcpy(ent_out, ent.p(), (size_t)n * ew * 8);
  hipsim::launch(dd::k_dedup_find, (unsigned)grid, (unsigned)dd::kThreads, (const unsigned long long*)ent.p(), n,
                 (const unsigned long long*)carry.p(), nc, window, (const int*)ord.p(), srecs.p(), dup.p());
  if (!all_ok()) return -1;
  if (!carry_same()) return -6;
  if (memcmp(ent.p(), ent_out, (size_t)n * ew * 8) != 0) return -1;            // ... and k_dedup_find only reads the entries
  memcpy(dup_out, dup.p(), (size_t)n * 4);
  memcpy(sorted_out, srecs.p(), (size_t)n * rw * 8);
  hipsim::launch(dd::k_dedup_merge, (unsigned)grid, (unsigned)dd::kThreads, (const unsigned long long*)carry.p(), nc,
                 (const unsigned long long*)ent.p(), n, horizon, merged.p(), state.p());
  if (!all_ok()) return -1;
  if (!carry_same()) return -6;
  if (memcmp(ent.p(), ent_out, (size_t)n * ew * 8) != 0) return -1;
  memcpy(merged_out, merged.p(), (size_t)(nc + n) * ew * 8);
  memcpy(state_out, state.p(), sizeof(dd::State));
  hipsim::launch(dd::k_dedup_mark, (unsigned)grid, (unsigned)dd::kThreads, (const int*)dup.p(), n, recs.p(), rows.p());
  if (!all_ok() || memcmp(dup.p(), dup_out, (size_t)n * 4) != 0) return -1;
  memcpy(recs_out, recs.p(), (size_t)n * rw * 8);
  memcpy(rows_out, rows.p(), (size_t)n * ww * 8);
  const dd::State s = state.p()[0];
  if (s.off < 0 || s.cnt < 1 || s.off + s.cnt != nc + n) return -6;
  return 0;
}
}
