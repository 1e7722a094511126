// mlat_rule_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  The twin of tests/sim/mlat_rule_driver.cpp on the GPU: the same entry
// point, sim_mlat_rule, with the same arguments and return codes, over the SHIPPED translation units
// gr_adsb_amd/csrc/adsb_mlat.hip and adsb_mlat_rule.hip -- each compiled as a unit of its own with the library's flags and
// linked beside this file into tests/gpu/libadsb_mlat_rule_dev.so (tests/test_gpu_mlat_rule_device.py builds it) -- and their
// real launchers launch_heads / launch_groups_rule / launch_solve_lm with their own cover().  mlat_device_driver.hip is included
// whole: its sticky HIP status, its call() (the phases, guards and carry back whole after each) and its sim_mlat, which
// ADSB_MLAT_SOLVER_GN is.  This file launches no kernel itself and includes no device code.  `grid` is accepted and ignored.
// Never linked into libadsb_hip.so.
#include "mlat_device_driver.hip"

#include "../../gr_adsb_amd/csrc/adsb_mlat_rule.h"
#include "../sim/mlat_rule_host_rule.h"

static_assert(mh::kAuxBytes == 32 && mh::kMinRxAided == 3, "the sizes adsb_mlat_rule.h states");

extern "C" {

int sim_mlat_aux_bytes() { return mh::kAuxBytes; }
unsigned long long sim_mlat_rule_layout_bytes(long long nc, long long n_streams) {
  return (unsigned long long)mh::layout_rule((size_t)nc, (size_t)n_streams).bytes;
}

// sim_mlat_rule (tests/sim/mlat_rule_driver.cpp), argument for argument; -38: dev_mlat_set_carry was not called.
int sim_mlat_rule(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, const double* rx, int n_streams,
                  double window, double t_lo, double t_hi, int solver, int flags, int min_rx, int reserved, double alt_weight, int grid,
                  int zero_hash, void* fixes, void* aux, int cap, int* n_fixes, int* member_stream, double* member_ts, int member_cap, int* n_members,
                  int* heads_out, int* n_heads) {
  if (mlat_rule::rule_refused(solver, flags, min_rx, reserved, alt_weight) || t_lo != t_lo || t_hi != t_hi || nc < 0 || n_streams < 0) return -22;
  if (solver == mlat_rule::kSolverGn) {
    const int rc = sim_mlat(ts, bits14, marker, stream, nc, rx, n_streams, window, t_lo, t_hi, min_rx, grid, zero_hash, fixes, cap, n_fixes,
                            member_stream, member_ts, member_cap, n_members, heads_out, n_heads);
    if (rc == 0 && aux)
      for (int k = 0; k < *n_fixes; ++k) {
        int* const a = (int*)((char*)aux + (size_t)k * mh::kAuxBytes);
        memset(a, 0, mh::kAuxBytes);
        a[4] = -1;                                    // alt_ft
      }
    return rc;
  }
  if (!g_carry) return -38;
  *n_fixes = 0; *n_members = 0;
  if (n_heads) *n_heads = 0;
  if (nc == 0) return 0;
  if (g_dead) return g_dead;
  std::vector<unsigned long long> words((size_t)nc * (mh::kEntBytes / 8), 0);
  g_carry(ts, bits14, marker, stream, nc, zero_hash, words.data());
  const mh::RuleLayout L = mh::layout_rule((size_t)nc, (size_t)n_streams);
  const auto solve = [&](hipStream_t st, const void* carry, int ng, void* work) {
    return mh::launch_solve_lm(st, carry, nc, ng, window, n_streams, flags, alt_weight, work, L);
  };
  return call(words.data(), nc, rx, n_streams, window, t_lo, t_hi, min_rx, mh::kMinRxAided, L, mlat_rule::parts_rule(L, (size_t)nc, (size_t)n_streams),
              mh::launch_groups_rule, solve, fixes, aux, mh::kAuxBytes, cap, n_fixes, member_stream, member_ts, member_cap, n_members, heads_out, n_heads);
}
}
