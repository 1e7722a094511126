// mlat_rule_driver.cpp -- TEST INFRASTRUCTURE ONLY.  adsb_stream_mlat_rule on the SIMT emulator: mlat_driver.cpp (included whole:
// its carry, its launches and its entry point sim_mlat are in this library too) plus sim_mlat_rule, which runs the damped
// path's kernels (gr_adsb_amd/csrc/adsb_mlat_rule_device.h) through mlat_driver.cpp's call(), with what differs stated here:
// the argument table, the work buffer carved by adsb_mlat_rule.h's layout_rule() before the first launch, the counts
// read between the phases, -ENOSPC decided before k_mlat_solve_lm with nothing written.  Every part of the work buffer has
// guard bytes behind it.  With ADSB_MLAT_SOLVER_GN the call is sim_mlat, as the host's is adsb_stream_mlat.  Its twin on the GPU
// is tests/gpu/mlat_rule_device_driver.hip; the two share mlat_rule_host_rule.h.  Never linked into libadsb_hip.so.
#include "mlat_driver.cpp"

#include "../../gr_adsb_amd/csrc/adsb_mlat_rule.h"
#include "../../gr_adsb_amd/csrc/adsb_mlat_rule_device.h"
#include "mlat_rule_host_rule.h"

static_assert(sizeof(ml::Aux) == mh::kAuxBytes && mlat_rule::kRestart == ml::kRuleRestart && mlat_rule::kAltitude == ml::kRuleAltitude,
              "the sizes and flags adsb_mlat_rule.h and the device code state");

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
  const mh::RuleLayout L = mh::layout_rule((size_t)nc, (size_t)n_streams);
  Work W(L, mlat_rule::parts_rule(L, (size_t)nc, (size_t)n_streams));
  const auto solve = [&](Work& w, const unsigned long long* c, unsigned g) {
    hipsim::launch(ml::k_mlat_solve_lm, g, (unsigned)ml::kThreads, c, nc, (const int*)w.at<int>(L.heads), (const int*)w.at<int>(L.gsel),
                   (const int*)w.at<int>(L.gfirst), (const int*)w.at<int>(L.tot_groups), window, (const double*)w.at<double>(L.rx), n_streams, flags,
                   alt_weight, w.at<ml::Fix>(L.fixes), w.at<ml::Aux>(L.aux), w.at<int>(L.member_stream), w.at<double>(L.member_ts));
  };
  return call(ts, bits14, marker, stream, nc, rx, n_streams, window, t_lo, t_hi, min_rx, mh::kMinRxAided, grid, zero_hash, W, ml::k_mlat_groups_rule, solve,
              fixes, aux, sizeof(ml::Aux), cap, n_fixes, member_stream, member_ts, member_cap, n_members, heads_out, n_heads);
}
}
