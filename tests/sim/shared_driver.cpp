// shared_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the shared decoder of a fleet (ADSB_FLAG_STREAM_DECODE_SHARED) on the
// SIMT emulator in hipsim.h, on host memory: the time order's kernels of gr_adsb_amd/csrc/adsb_shared_device.h (k_shared_keys,
// k_shared_sort_*, k_shared_gather, k_shared_scatter) around fleet_driver.cpp's decode step (its Fleet, rehash and
// decode_step: the growth rule, the k_fleet_* kernels and the bookkeeping, here with one item and everything under stream
// index 0), in the order adsb_hip.hip's fleet_step queues them on a shared context.  The host's own code runs only in
// tests/test_gpu_shared_decode.py.  Never linked into libadsb_hip.so.
#include "fleet_driver.cpp"

inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, sizeof r); return r; }

#include "../../gr_adsb_amd/csrc/adsb_shared_device.h"

namespace sh = adsb_shared;

static_assert(sizeof(Rec) == sh::kRecWords * 8 && sizeof(DecRow) == sh::kRowWords * 8, "the sizes adsb_shared_device.h assumes");

namespace {
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
  return open_fleet(n_streams, slots, fec, all, ages != 0, fs);
}
void sim_shared_close(void* h) { delete (Fleet*)h; }
void sim_shared_set_start(void* h, int stream, double start) { ((Fleet*)h)->start[(size_t)stream] = start; }
void sim_shared_set_max_cap(void* h, long long cap) { ((Fleet*)h)->max_cap = cap; }
// adsb_streams_decoder_reset: a new generation of index 0
void sim_shared_reset(void* h) { (void)reset_stream(*(Fleet*)h, 0); }
void sim_shared_stats(void* h, long long* planes, long long* cap, long long* grows, long long* used) {
  const Fleet& F = *(Fleet*)h;
  *planes = F.live_planes; *cap = F.st.cap; *grows = F.grows; *used = F.used;
}
// a digest of the whole state: the store's arrays byte for byte, in slot order, and the books
unsigned long long sim_shared_digest(void* h) {
  Fleet& F = *(Fleet*)h;
  unsigned long long d = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { d ^= ((const unsigned char*)p)[i]; d *= 1099511628211ull; } };
  mix(F.st.keys.p(), (size_t)F.st.cap * 8); mix(F.st.ann.p(), (size_t)F.st.cap * 8);
  mix(F.st.planes.p(), (size_t)F.st.cap * sizeof(Plane));
  if (F.ages) mix(F.st.seen.p(), (size_t)F.st.cap * 8);
  const long long books[6] = {F.live_slots, F.live_planes, F.used, F.grows, (long long)F.call, (long long)F.gen[0]};
  mix(books, sizeof books);
  return d;
}
// the decoder's planes read from the store itself: addresses and last_seen clocks (0 without ages; cap entries at the most)
// -> their number
int sim_shared_planes(void* h, int* addr, long long* seen, int cap) {
  Fleet& F = *(Fleet*)h;
  int k = 0;
  for (long long i = 0; i < F.st.cap; ++i) {
    const unsigned long long key = F.st.keys.p()[i];
    if (key == kFleetEmpty || (key >> kFleetAddrBits) != (key_base(F, 0) >> kFleetAddrBits)) continue;
    if (!(F.st.planes.p()[i].present & kHasPlane)) continue;
    if (k < cap) { addr[k] = (int)(key & 0xFFFFFFu); seen[k] = F.ages ? F.st.seen.p()[i] : 0; }
    ++k;
  }
  return k;
}
// adsb_stream_planes_expire for the one decoder: its planes with last_seen < cutoff are dropped by a rehash
long long sim_shared_expire(void* h, long long cutoff, int grid) {
  Fleet& F = *(Fleet*)h;
  const std::vector<long long> cut(F.gen.size(), cutoff);
  long long removed = 0;
  const int r = rehash(F, F.st.cap, grid, false, cut.data(), &removed);
  for (size_t s = 1; s < F.gen.size(); ++s) if (F.slots[s] || F.planes[s]) return -3;     // nobody but stream 0 holds anything
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
  Fleet& F = *(Fleet*)h;
  if (n <= 0) return 0;
  if (n_items <= 0 || item_first[n_items] != n) return -5;
  for (int i = 0; i < n_items; ++i)
    if (item_stream[i] < 0 || (size_t)item_stream[i] >= F.gen.size() || item_first[i] > item_first[i + 1]) return -5;
  Guarded<unsigned char> b14((size_t)n * 14, 0);
  memcpy(b14.p(), bits14, (size_t)n * 14);
  Guarded<Rec> recs;
  int r;
  if ((r = build_recs(b14, offset, dem, n, F.fec, grid, recs))) return r;
  // the time order (its kernels touch neither the store nor the books: a call refused below has changed nothing)
  Guarded<int> first((size_t)n_items + 1, 0);
  Guarded<double> start((size_t)n_items, 0);
  for (int i = 0; i <= n_items; ++i) first.p()[i] = item_first[i];
  for (int i = 0; i < n_items; ++i) start.p()[i] = F.start[(size_t)item_stream[i]];
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
  // the decode step on the time-ordered list: one item of stream 0, the true timestamps over the one item's
  Guarded<FleetItem> items(2, 0);
  items.p()[0].base = key_base(F, 0);
  items.p()[1].first = n; items.p()[1].stream = -1;
  const int book = 0;
  if ((r = decode_step(F, srecs, n, items, 1, &book, ts_sorted.p(), grid, srows))) return r;
  hipsim::launch(sh::k_shared_scatter, (unsigned)grid, (unsigned)sh::kThreads, (const unsigned long long*)srecs.p(),
                 (const unsigned long long*)srows.p(), (const int*)order.p(), n, (unsigned long long*)recs.p(), (unsigned long long*)rows.p());
  if (!srecs.ok() || !srows.ok() || !recs.ok() || !rows.ok() || !order.ok()) return -1;
  for (int t = 0; t < n; ++t) flags_out[t] = (unsigned short)(recs.p()[t].w[3] >> 48);
  memcpy(rows_out, rows.p(), (size_t)n * sizeof(DecRow));
  memcpy(order_out, order.p(), (size_t)n * sizeof(int));
  memcpy(ts_out, ts.p(), (size_t)n * sizeof(double));
  return 0;
}
}
