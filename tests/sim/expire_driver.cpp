// expire_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the plane ages (ADSB_FLAG_PLANE_AGES; gr_adsb_amd/csrc/adsb_device.h:
// k_ages_fold, k_fleet_fold with FleetArgs::seen set, k_ages_expire, k_ages_emit, k_ages_rehash,
// k_ages_store_emit) on the SIMT emulator in hipsim.h, on host memory, in the order adsb_hip.hip queues them.  The
// decoders and snapshots are those of decode_driver.cpp, fleet_driver.cpp and planes_driver.cpp, called here with a
// last_seen array: a fleet opened here is fleet_driver.cpp's Fleet with the clocks beside its store's slots, and every
// sim_fleet_* / sim_planes_* entry point takes it.  The host code itself runs only in tests/test_gpu_expire.py.
// Never linked into libadsb_hip.so.
#include "planes_driver.cpp"

#include <climits>

extern "C" {

// ---- one decoder ---------------------------------------------------------------------------------------------------------------
// sim_dec_pdus with the last_seen array (2^24 int64, never cleared: any bytes at first); seen null: as sim_dec_pdus
int sim_exp_dec_pdus(unsigned char* bits14, const double* ts, int n, int grid, unsigned long long* table, void* st, void* planes,
                     long long* seen, unsigned epoch, unsigned long long pass, int fec, int all, void* rows) {
  return dec_pdus(bits14, ts, n, grid, table, st, planes, seen, epoch, pass, fec, all, rows);
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
  return planes_dense(table, planes, seen, epoch, lo, hi, grid, cap, rows, seen_out, n_out);
}

// ---- the fleet -----------------------------------------------------------------------------------------------------------------
void* sim_exp_fleet_open(int n_streams, long long slots, int fec, int all) { return open_fleet(n_streams, slots, fec, all, true, 1.0); }
void sim_exp_fleet_close(void* h) { sim_fleet_close(h); }
int sim_exp_fleet_reset(void* h, int stream) { return sim_fleet_reset(h, stream); }
// the slot of (stream, addr) in its current generation, -1 if none (for tests that build probe clusters)
long long sim_exp_fleet_slot_of(void* h, int stream, unsigned addr) {
  Fleet& F = *(Fleet*)h;
  bool claimed = false;
  const unsigned s = fleet_slot(F.st.view(), key_base(F, (size_t)stream) | addr, false, &claimed);
  return s == kFleetNone ? -1 : (long long)s;
}
// the home slot of (stream, addr) in a store of cap slots
unsigned sim_exp_fleet_home(void* h, int stream, unsigned addr, long long cap) {
  return fleet_hash(key_base(*(Fleet*)h, (size_t)stream) | addr) & (unsigned)(cap - 1);
}

// sim_fleet_call with the last_seen array (return values as there)
int sim_exp_fleet_call(void* h, const unsigned char* bits14, const double* ts, const int* stream, int n, int grid, void* rows_out) {
  return sim_fleet_call(h, bits14, ts, stream, n, grid, rows_out);
}

// adsb_stream_planes_expire: streams null (all; cutoffs[n_streams]) or n_sel strictly ascending indices (cutoffs[n_sel]).
// 0; -22: bad indices or cutoffs missing; -1 / -3 as the rehash
int sim_exp_fleet_expire(void* h, const int* streams, int n_sel, const long long* cutoffs, int grid, long long* n_removed) {
  Fleet& F = *(Fleet*)h;
  if (!F.ages || select_streams(F, streams, &n_sel, nullptr) || (n_sel > 0 && !cutoffs)) return kInvalid;
  std::vector<long long> cut(F.gen.size(), LLONG_MIN);
  for (int i = 0; i < n_sel; ++i) cut[streams ? (size_t)streams[i] : (size_t)i] = cutoffs[i];
  return rehash(F, F.st.cap, grid, false, cut.data(), n_removed);
}

// adsb_stream_planes_seen: sim_planes_fleet with k_ages_store_emit; rows / seen_out may be null
int sim_exp_fleet_seen(void* h, const int* streams, int n_sel, int grid, int cap, void* rows, long long* seen_out, int* first,
                       int* n_out) {
  return planes_fleet(*(Fleet*)h, streams, n_sel, true, grid, cap, rows, seen_out, first, n_out);
}
}
