// mlat_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs adsb_stream_mlat's kernels (gr_adsb_amd/csrc/adsb_mlat_device.h) on the SIMT
// emulator in hipsim.h, on host memory, over a carry the caller states entry by entry, in the order adsb_mlat.hip queues them
// and with the host's rule of adsb_hip.hip restated, once, in call() (mlat_rule_driver.cpp runs the damped path through it
// too): the work buffer is carved by adsb_mlat.h's layout() before the first
// launch, the head count and then the group and member counts are read between the phases, -ENOSPC is decided before
// k_mlat_solve and writes nothing.  Every part of the work buffer has guard bytes behind it.  The host's own code runs only in
// tests/test_gpu_mlat.py.  Its twin is tests/gpu/mlat_device_driver.hip: the same entry point, sim_mlat, over the shipped
// translation unit and its real launchers on the GPU (tests/test_gpu_mlat_device.py); the two share mlat_host_rule.h -- the
// parts, the guards and the counts' range checks -- and the carry's words, which sim_mlat_carry below hands to the device
// driver, so that both see identical bytes.  Never linked into libadsb_hip.so.
#include "hipsim.h"

#include <vector>

inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, sizeof r); return r; }
inline double __longlong_as_double(long long v) { double r; memcpy(&r, &v, sizeof r); return r; }

#include "../../gr_adsb_amd/csrc/adsb_dedup_device.h"
#include "../../gr_adsb_amd/csrc/adsb_mlat.h"
#include "../../gr_adsb_amd/csrc/adsb_mlat_device.h"
#include "mlat_host_rule.h"

namespace ml = adsb_mlat;
namespace mh = adsb_mlat_host;

static_assert(sizeof(ml::Fix) == mh::kFixBytes && ml::kEntWords == adsb_dedup::kEntWords && mh::kChunk == ml::kThreads, "the sizes adsb_mlat.h states");

namespace {
using mlat_rule::kGuard;
using mlat_rule::kTail;

// the carry's entries as k_dedup_entries writes them; zero_hash: every hash 0, so that only the payload words can tell two
// replies apart
std::vector<unsigned long long> make_carry(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, bool zero_hash) {
  std::vector<unsigned long long> c((size_t)nc * ml::kEntWords + 1, 0);      // (+1: data() is never null)
  for (int i = 0; i < nc; ++i) {
    unsigned long long w2 = 0, w3 = 0;
    memcpy(&w2, bits14 + (size_t)i * 14, 8);
    memcpy(&w3, bits14 + (size_t)i * 14 + 8, 6);
    const int mk = marker[i];
    const unsigned long long a = mk == 0 ? 0ull : mk == 2 ? w2 : (w2 & 0x00FFFFFFFFFFFFFFull);
    const unsigned long long b = mk == 2 ? w3 : 0ull;
    unsigned long long* e = &c[(size_t)i * ml::kEntWords];
    memcpy(&e[0], &ts[i], 8);
    e[1] = a; e[2] = b;
    e[3] = (unsigned long long)(zero_hash ? 0u : adsb_dedup::hash32(a, b)) | ((unsigned long long)((unsigned)stream[i] & 0xFFFFFFu) << 32) |
           ((unsigned long long)mk << 56);
  }
  return c;
}

struct Work {
  mh::Layout L;
  std::vector<unsigned char> raw;
  std::vector<std::pair<size_t, size_t>> parts;      // offset, bytes in use
  Work(const mh::Layout& l, std::vector<std::pair<size_t, size_t>> p) : L(l), raw(l.bytes + kTail, kGuard), parts(std::move(p)) {}
  template <class T> T* at(size_t off) { return (T*)(raw.data() + off); }
  bool ok() const { return mlat_rule::guards_ok(raw.data(), raw.size(), parts); }
};

unsigned cover(long long work, int per, int grid) {
  const long long g = (work + per - 1) / per;
  return (unsigned)(grid > 0 ? grid : g < 1 ? 1 : g);
}

void compact(Work& W, const int* w, const int* span, int min_w, int* tot, int add_lo, int* idx, int* first, int grid) {
  const unsigned g = (unsigned)(grid > 0 ? grid : 2);
  hipsim::launch(ml::k_mlat_count, g, (unsigned)ml::kThreads, w, span, min_w, W.at<int>(W.L.cnt), W.at<int>(W.L.sum));
  hipsim::launch(ml::k_mlat_scan, 1u, (unsigned)ml::kThreads, span, W.at<int>(W.L.cnt), W.at<int>(W.L.sum), tot);
  hipsim::launch(ml::k_mlat_place, g, (unsigned)ml::kThreads, w, span, min_w, (const int*)W.at<int>(W.L.cnt), (const int*)W.at<int>(W.L.sum), add_lo,
                 idx, first);
}

// k_mlat_groups or k_mlat_groups_rule
typedef void (*groups_kernel)(const unsigned long long*, int, const int*, const int*, double, const double*, int, int*);

// One call over the carry, after the entry point's argument table: the launches in the host's order on the work buffer W (carved
// and given its parts by the caller), the counts read between the phases with min_group in their range check, -ENOSPC before
// the solve.  groups and solve(W, carry, grid of the solve kernel) are what differs between adsb_stream_mlat and
// adsb_stream_mlat_rule's damped path; aux (may be null): aux_row_bytes per fix from W.L.aux.
template <class Solve>
int call(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, const double* rx, int n_streams, double window,
         double t_lo, double t_hi, int min_rx, int min_group, int grid, int zero_hash, Work& W, groups_kernel groups, Solve solve, void* fixes, void* aux,
         size_t aux_row_bytes, int cap, int* n_fixes, int* member_stream, double* member_ts, int member_cap, int* n_members, int* heads_out,
         int* n_heads) {
  const std::vector<unsigned long long> carry = make_carry(ts, bits14, marker, stream, nc, zero_hash != 0), before = carry;
  memcpy(W.at<double>(W.L.rx), rx, (size_t)n_streams * 24);
  const unsigned long long* c = carry.data();
  int* const range = W.at<int>(W.L.range);
  hipsim::launch(ml::k_mlat_range, 1u, (unsigned)ml::kWave, c, nc, t_lo, t_hi, range);
  hipsim::launch(ml::k_mlat_heads, cover(nc, ml::kThreads, grid), (unsigned)ml::kThreads, c, nc, (const int*)range, window, W.at<int>(W.L.w));
  compact(W, W.at<int>(W.L.w), range, 1, W.at<int>(W.L.tot_heads), 1, W.at<int>(W.L.heads), nullptr, grid);
  if (!W.ok() || carry != before) return -1;
  const int nh = W.at<int>(W.L.tot_heads)[1];
  if (!mlat_rule::heads_in_range(nh, nc)) return -5;
  if (n_heads) *n_heads = nh;
  if (heads_out) memcpy(heads_out, W.at<int>(W.L.heads), (size_t)nh * 4);
  if (nh == 0) return 0;
  const int* const hspan = W.at<int>(W.L.tot_heads);
  hipsim::launch(groups, cover(nh, ml::kWaves, grid), (unsigned)ml::kThreads, c, nc, (const int*)W.at<int>(W.L.heads), hspan, window,
                 (const double*)W.at<double>(W.L.rx), n_streams, W.at<int>(W.L.nrx));
  compact(W, W.at<int>(W.L.nrx), hspan, min_rx, W.at<int>(W.L.tot_groups), 0, W.at<int>(W.L.gsel), W.at<int>(W.L.gfirst), grid);
  if (!W.ok() || carry != before) return -1;
  const int ng = W.at<int>(W.L.tot_groups)[1], nm = W.at<int>(W.L.tot_groups)[2];
  if (!mlat_rule::groups_in_range(ng, nm, nc, min_rx, min_group)) return -5;
  *n_fixes = ng; *n_members = nm;
  if (ng > cap || nm > member_cap) return -28;
  if (ng == 0) return 0;
  solve(W, c, cover(ng, ml::kWaves, grid));
  if (!W.ok() || carry != before) return -1;
  memcpy(fixes, W.at<ml::Fix>(W.L.fixes), (size_t)ng * sizeof(ml::Fix));
  if (aux) memcpy(aux, W.at<unsigned char>(W.L.aux), (size_t)ng * aux_row_bytes);
  memcpy(member_stream, W.at<int>(W.L.member_stream), (size_t)nm * 4);
  memcpy(member_ts, W.at<double>(W.L.member_ts), (size_t)nm * 8);
  return 0;
}
}  // namespace

extern "C" {

int sim_mlat_tile() { return ml::kTile; }
int sim_mlat_lds_bytes(int which) { return which == 0 ? ml::kHeadsLdsBytes : which == 1 ? ml::kPlaceLdsBytes : ml::kScanLdsBytes; }
int sim_mlat_fix_bytes() { return (int)sizeof(ml::Fix); }
unsigned long long sim_mlat_layout_bytes(long long nc, long long n_streams) { return (unsigned long long)mh::layout((size_t)nc, (size_t)n_streams).bytes; }

// The carry's words as sim_mlat builds them, into out_words[4 nc]: what tests/gpu/mlat_device_driver.hip is given.
void sim_mlat_carry(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, int zero_hash,
                    unsigned long long* out_words) {
  if (nc <= 0) return;
  const std::vector<unsigned long long> c = make_carry(ts, bits14, marker, stream, nc, zero_hash != 0);
  memcpy(out_words, c.data(), (size_t)nc * ml::kEntWords * 8);
}

// One adsb_stream_mlat call over the carry ts / bits14 / marker / stream [nc] (in carry order; marker 0: takes no part, 1: 56
// bits, 2: 112 bits) with rx[3 n_streams] (NaN: no position).  heads_out (may be null, nc ints): the heads of the range, their
// number in *n_heads.  Returns 0, -28 (-ENOSPC: the counts are stated, nothing is written), -22 (arguments), -1: a guard was
// overwritten or the carry was written, -5: a count out of range.
int sim_mlat(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, const double* rx, int n_streams,
             double window, double t_lo, double t_hi, int min_rx, int grid, int zero_hash, void* fixes, int cap, int* n_fixes, int* member_stream,
             double* member_ts, int member_cap, int* n_members, int* heads_out, int* n_heads) {
  if (min_rx < mh::kMinRx || t_lo != t_lo || t_hi != t_hi || nc < 0) return -22;
  *n_fixes = 0; *n_members = 0;
  if (n_heads) *n_heads = 0;
  if (nc == 0) return 0;
  const mh::Layout L = mh::layout((size_t)nc, (size_t)n_streams);
  Work W(L, mlat_rule::parts(L, (size_t)nc, (size_t)n_streams));
  const auto solve = [&](Work& w, const unsigned long long* c, unsigned g) {
    hipsim::launch(ml::k_mlat_solve, g, (unsigned)ml::kThreads, c, nc, (const int*)w.at<int>(L.heads), (const int*)w.at<int>(L.gsel),
                   (const int*)w.at<int>(L.gfirst), (const int*)w.at<int>(L.tot_groups), window, (const double*)w.at<double>(L.rx), n_streams,
                   w.at<ml::Fix>(L.fixes), w.at<int>(L.member_stream), w.at<double>(L.member_ts));
  };
  return call(ts, bits14, marker, stream, nc, rx, n_streams, window, t_lo, t_hi, min_rx, mh::kMinRx, grid, zero_hash, W, ml::k_mlat_groups, solve, fixes,
              nullptr, 0, cap, n_fixes, member_stream, member_ts, member_cap, n_members, heads_out, n_heads);
}
}
