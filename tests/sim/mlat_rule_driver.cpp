// mlat_rule_driver.cpp -- TEST INFRASTRUCTURE ONLY.  adsb_stream_mlat_rule on the SIMT emulator: mlat_driver.cpp (included whole:
// its carry, its launches and its entry point sim_mlat are in this library too) plus sim_mlat_rule, which runs the damped
// path's kernels (gr_adsb_amd/csrc/adsb_mlat_rule_device.h) in the order adsb_hip.hip queues them and with the host's rule
// restated: the argument table, the work buffer carved by adsb_mlat_rule.h's layout_rule() before the first launch, the counts
// read between the phases, -ENOSPC decided before k_mlat_solve_lm with nothing written.  Every part of the work buffer has
// guard bytes behind it.  With ADSB_MLAT_SOLVER_GN the call is sim_mlat, as the host's is adsb_stream_mlat.  Its twin on the GPU
// is tests/gpu/mlat_rule_device_driver.hip; the two share mlat_rule_host_rule.h.  Never linked into libadsb_hip.so.
#include "mlat_driver.cpp"

#include "../../gr_adsb_amd/csrc/adsb_mlat_rule.h"
#include "../../gr_adsb_amd/csrc/adsb_mlat_rule_device.h"
#include "mlat_rule_host_rule.h"

static_assert(sizeof(ml::Aux) == mh::kAuxBytes && mlat_rule::kRestart == ml::kRuleRestart && mlat_rule::kAltitude == ml::kRuleAltitude,
              "the sizes and flags adsb_mlat_rule.h and the device code state");

namespace {
struct RuleWork {
  mh::RuleLayout L;
  std::vector<unsigned char> raw;
  std::vector<std::pair<size_t, size_t>> parts;
  RuleWork(size_t nc, size_t n_streams) : L(mh::layout_rule(nc, n_streams)), parts(mlat_rule::parts_rule(L, nc, n_streams)) {
    raw.assign(L.bytes + kTail, kGuard);
  }
  template <class T> T* at(size_t off) { return (T*)(raw.data() + off); }
  bool ok() const { return mlat_rule::guards_ok(raw.data(), raw.size(), parts); }
};

void compact_rule(RuleWork& W, const int* w, const int* span, int min_w, int* tot, int add_lo, int* idx, int* first, int grid) {
  const unsigned g = (unsigned)(grid > 0 ? grid : 2);
  hipsim::launch(ml::k_mlat_count, g, (unsigned)ml::kThreads, w, span, min_w, W.at<int>(W.L.cnt), W.at<int>(W.L.sum));
  hipsim::launch(ml::k_mlat_scan, 1u, (unsigned)ml::kThreads, span, W.at<int>(W.L.cnt), W.at<int>(W.L.sum), tot);
  hipsim::launch(ml::k_mlat_place, g, (unsigned)ml::kThreads, w, span, min_w, (const int*)W.at<int>(W.L.cnt), (const int*)W.at<int>(W.L.sum), add_lo,
                 idx, first);
}
}  // namespace

extern "C" {

int sim_mlat_aux_bytes() { return (int)sizeof(ml::Aux); }
unsigned long long sim_mlat_rule_layout_bytes(long long nc, long long n_streams) {
  return (unsigned long long)mh::layout_rule((size_t)nc, (size_t)n_streams).bytes;
}
// the altitude k_mlat_solve_lm reads from a payload: the device function itself, called on the host
int sim_mlat_alt_ft(const unsigned char* bits14) {
  unsigned long long a = 0;
  memcpy(&a, bits14, 8);
  return ml::mlat_alt_ft(a);
}

// One adsb_stream_mlat_rule call; sim_mlat's arguments, the rule's four fields and alt_weight, and aux (may be null; `cap` rows).
// Returns as sim_mlat does; -22 also by the rule's argument table.
int sim_mlat_rule(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, const double* rx, int n_streams,
                  double window, double t_lo, double t_hi, int solver, int flags, int min_rx, int reserved, double alt_weight, int grid,
                  int zero_hash, void* fixes, void* aux, int cap, int* n_fixes, int* member_stream, double* member_ts, int member_cap, int* n_members,
                  int* heads_out, int* n_heads) {
  if (mlat_rule::rule_refused(solver, flags, min_rx, reserved, alt_weight) || t_lo != t_lo || t_hi != t_hi || nc < 0) return -22;
  if (solver == mlat_rule::kSolverGn) {
    const int rc = sim_mlat(ts, bits14, marker, stream, nc, rx, n_streams, window, t_lo, t_hi, min_rx, grid, zero_hash, fixes, cap, n_fixes,
                            member_stream, member_ts, member_cap, n_members, heads_out, n_heads);
    if (rc == 0 && aux) {
      ml::Aux* const a = (ml::Aux*)aux;
      for (int k = 0; k < *n_fixes; ++k) { memset(&a[k], 0, sizeof a[k]); a[k].alt_ft = -1; }
    }
    return rc;
  }
  *n_fixes = 0; *n_members = 0;
  if (n_heads) *n_heads = 0;
  if (nc == 0) return 0;
  const std::vector<unsigned long long> carry = make_carry(ts, bits14, marker, stream, nc, zero_hash != 0), before = carry;
  RuleWork W((size_t)nc, (size_t)n_streams);
  memcpy(W.at<double>(W.L.rx), rx, (size_t)n_streams * 24);
  const unsigned long long* c = carry.data();
  int* const range = W.at<int>(W.L.range);
  hipsim::launch(ml::k_mlat_range, 1u, (unsigned)ml::kWave, c, nc, t_lo, t_hi, range);
  hipsim::launch(ml::k_mlat_heads, cover(nc, ml::kThreads, grid), (unsigned)ml::kThreads, c, nc, (const int*)range, window, W.at<int>(W.L.w));
  compact_rule(W, W.at<int>(W.L.w), range, 1, W.at<int>(W.L.tot_heads), 1, W.at<int>(W.L.heads), nullptr, grid);
  if (!W.ok() || carry != before) return -1;
  const int nh = W.at<int>(W.L.tot_heads)[1];
  if (!mlat_rule::heads_in_range(nh, nc)) return -5;
  if (n_heads) *n_heads = nh;
  if (heads_out) memcpy(heads_out, W.at<int>(W.L.heads), (size_t)nh * 4);
  if (nh == 0) return 0;
  const int* const hspan = W.at<int>(W.L.tot_heads);
  hipsim::launch(ml::k_mlat_groups_rule, cover(nh, ml::kWaves, grid), (unsigned)ml::kThreads, c, nc, (const int*)W.at<int>(W.L.heads), hspan, window,
                 (const double*)W.at<double>(W.L.rx), n_streams, W.at<int>(W.L.nrx));
  compact_rule(W, W.at<int>(W.L.nrx), hspan, min_rx, W.at<int>(W.L.tot_groups), 0, W.at<int>(W.L.gsel), W.at<int>(W.L.gfirst), grid);
  if (!W.ok() || carry != before) return -1;
  const int ng = W.at<int>(W.L.tot_groups)[1], nm = W.at<int>(W.L.tot_groups)[2];
  if (!mlat_rule::groups_in_range_rule(ng, nm, nc, min_rx)) return -5;
  *n_fixes = ng; *n_members = nm;
  if (ng > cap || nm > member_cap) return -28;
  if (ng == 0) return 0;
  hipsim::launch(ml::k_mlat_solve_lm, cover(ng, ml::kWaves, grid), (unsigned)ml::kThreads, c, nc, (const int*)W.at<int>(W.L.heads),
                 (const int*)W.at<int>(W.L.gsel), (const int*)W.at<int>(W.L.gfirst), (const int*)W.at<int>(W.L.tot_groups), window,
                 (const double*)W.at<double>(W.L.rx), n_streams, flags, alt_weight, W.at<ml::Fix>(W.L.fixes), W.at<ml::Aux>(W.L.aux),
                 W.at<int>(W.L.member_stream), W.at<double>(W.L.member_ts));
  if (!W.ok() || carry != before) return -1;
  memcpy(fixes, W.at<ml::Fix>(W.L.fixes), (size_t)ng * sizeof(ml::Fix));
  if (aux) memcpy(aux, W.at<ml::Aux>(W.L.aux), (size_t)ng * sizeof(ml::Aux));
  memcpy(member_stream, W.at<int>(W.L.member_stream), (size_t)nm * 4);
  memcpy(member_ts, W.at<double>(W.L.member_ts), (size_t)nm * 8);
  return 0;
}
}
