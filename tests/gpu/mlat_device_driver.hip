// mlat_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  The twin of tests/sim/mlat_driver.cpp on the GPU: the same entry point,
// sim_mlat, with the same arguments and return codes, over the SHIPPED translation unit gr_adsb_amd/csrc/adsb_mlat.hip --
// compiled as a unit of its own with the library's flags and linked beside this file into tests/gpu/libadsb_mlat_dev.so
// (tests/test_gpu_mlat_device.py builds it) -- and its real launchers launch_heads / launch_groups / launch_solve with their own
// cover().  This file launches no k_mlat_* kernel itself and includes no device code.
//
// `grid` is accepted and IGNORED: the real launchers choose the grid.  The emulator driver's grid cases therefore run here
// twice with equal effect.
//
// The carry and the work buffer (adsb_mlat.h's layout(), filled with the guard byte first, a guard tail behind the last part)
// live in device memory.  Between the phases the host does what adsb_stream_mlat does: it reads the head count, then the
// group and member counts, with the range checks of mlat_host_rule.h -- adsb_stream_mlat's own expressions, -5 here -- and
// decides -ENOSPC before launch_solve, writing nothing.  After each phase the work buffer and the carry come back whole: a
// guard byte or a carry byte that changed is -1.  Every HIP call's status is checked: an error is -1000 - hipError_t, no
// further GPU call is made, and every later call of this library returns the same code at once.
//
// The carry's words are not built here (hash32 is device code): dev_mlat_words takes them, and sim_mlat gets them from the
// function dev_mlat_set_carry was given -- the emulator driver's sim_mlat_carry, so that both drivers see identical bytes.
// Never linked into libadsb_hip.so.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_mlat.h"
#include "../sim/mlat_host_rule.h"

namespace mh = adsb_mlat_host;

static_assert(mh::kEntBytes == 32 && mh::kFixBytes == 88 && mh::kChunk == 256 && mh::kMinRx == 4, "the sizes adsb_mlat.h states");

namespace {
using mlat_rule::kGuard;
using mlat_rule::kTail;

typedef void (*carry_fn)(const double*, const unsigned char*, const int*, const int*, int, int, unsigned long long*);
carry_fn g_carry = nullptr;
int g_dead = 0;                                       // the first HIP error's code: nothing is queued after it

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p && !g_dead) (void)hipFree(p); }
};

// the status of one HIP call -> 0, or the sticky code
int hip_rc(hipError_t e) {
  if (e != hipSuccess && !g_dead) g_dead = -1000 - (int)e;
  return g_dead;
}
#define HIP_OR_RETURN(call) do { if (hip_rc(call)) return g_dead; } while (0)

// after a phase: the launches' status, then the work buffer and the carry back whole -> 0, -1, or a HIP code
int phase_end(int launched, const DevBuf& d_work, std::vector<unsigned char>& raw, const std::vector<std::pair<size_t, size_t>>& parts,
              const DevBuf& d_carry, const unsigned long long* words, std::vector<unsigned long long>& back) {
  HIP_OR_RETURN((hipError_t)launched);
  HIP_OR_RETURN(hipMemcpy(raw.data(), d_work.p, raw.size(), hipMemcpyDeviceToHost));      // (waits for the null stream's kernels)
  HIP_OR_RETURN(hipMemcpy(back.data(), d_carry.p, back.size() * 8, hipMemcpyDeviceToHost));
  HIP_OR_RETURN(hipGetLastError());
  if (!mlat_rule::guards_ok(raw.data(), raw.size(), parts) || memcmp(back.data(), words, back.size() * 8) != 0) return -1;
  return 0;
}
// launch_groups or launch_groups_rule
typedef int (*groups_launcher)(void*, const void*, int, int, double, int, int, void*, const mh::Layout&);

// One call over words[4 nc], after the entry point's argument table, on a work buffer carved as L with `parts`: the real
// launchers in the host's order, phase_end behind each, the counts' range checks (min_group in the groups') and -ENOSPC before
// the solve.  groups and solve(stream, carry, work) -> the launch's status are what differs between adsb_stream_mlat and
// adsb_stream_mlat_rule's damped path; aux (may be null): aux_row_bytes per fix from L.aux.
template <class Solve>
int call(const unsigned long long* words, int nc, const double* rx, int n_streams, double window, double t_lo, double t_hi, int min_rx, int min_group,
         const mh::Layout& L, const std::vector<std::pair<size_t, size_t>>& parts, groups_launcher groups, Solve solve, void* fixes, void* aux,
         size_t aux_row_bytes, int cap, int* n_fixes, int* member_stream, double* member_ts, int member_cap, int* n_members, int* heads_out,
         int* n_heads) {
  std::vector<unsigned char> raw(L.bytes + kTail, kGuard);
  std::vector<unsigned long long> back((size_t)nc * (mh::kEntBytes / 8));
  DevBuf d_carry, d_work;
  HIP_OR_RETURN(hipMalloc(&d_carry.p, back.size() * 8));
  HIP_OR_RETURN(hipMalloc(&d_work.p, raw.size()));
  HIP_OR_RETURN(hipMemcpy(d_carry.p, words, back.size() * 8, hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemset(d_work.p, kGuard, raw.size()));
  if (n_streams > 0) HIP_OR_RETURN(hipMemcpy((char*)d_work.p + L.rx, rx, (size_t)n_streams * 24, hipMemcpyHostToDevice));
  const hipStream_t st = nullptr;
  const auto ints = [&](size_t off) { return (const int*)(raw.data() + off); };
  int rc;

  if ((rc = phase_end(mh::launch_heads(st, d_carry.p, nc, t_lo, t_hi, window, d_work.p, L), d_work, raw, parts, d_carry, words, back))) return rc;
  const int nh = ints(L.tot_heads)[1];
  if (!mlat_rule::heads_in_range(nh, nc)) return -5;
  if (n_heads) *n_heads = nh;
  if (heads_out) memcpy(heads_out, ints(L.heads), (size_t)nh * 4);
  if (nh == 0) return 0;

  if ((rc = phase_end(groups(st, d_carry.p, nc, nh, window, min_rx, n_streams, d_work.p, L), d_work, raw, parts, d_carry, words, back))) return rc;
  const int ng = ints(L.tot_groups)[1], nm = ints(L.tot_groups)[2];
  if (!mlat_rule::groups_in_range(ng, nm, nc, min_rx, min_group)) return -5;
  *n_fixes = ng; *n_members = nm;
  if (ng > cap || nm > member_cap) return -28;
  if (ng == 0) return 0;

  if ((rc = phase_end(solve(st, d_carry.p, ng, d_work.p), d_work, raw, parts, d_carry, words, back))) return rc;
  memcpy(fixes, raw.data() + L.fixes, (size_t)ng * mh::kFixBytes);
  if (aux) memcpy(aux, raw.data() + L.aux, (size_t)ng * aux_row_bytes);
  memcpy(member_stream, raw.data() + L.member_stream, (size_t)nm * 4);
  memcpy(member_ts, raw.data() + L.member_ts, (size_t)nm * 8);
  return 0;
}
}  // namespace

extern "C" {

int sim_mlat_fix_bytes() { return mh::kFixBytes; }
unsigned long long sim_mlat_layout_bytes(long long nc, long long n_streams) { return (unsigned long long)mh::layout((size_t)nc, (size_t)n_streams).bytes; }
void dev_mlat_set_carry(carry_fn f) { g_carry = f; }
int dev_mlat_dead() { return g_dead; }

// sim_mlat (tests/sim/mlat_driver.cpp) over words[4 nc], the carry's entries as the emulator driver's sim_mlat_carry states them
int dev_mlat_words(const unsigned long long* words, int nc, const double* rx, int n_streams, double window, double t_lo, double t_hi, int min_rx,
                   void* fixes, int cap, int* n_fixes, int* member_stream, double* member_ts, int member_cap, int* n_members, int* heads_out,
                   int* n_heads) {
  if (min_rx < mh::kMinRx || t_lo != t_lo || t_hi != t_hi || nc < 0 || n_streams < 0) return -22;
  *n_fixes = 0; *n_members = 0;
  if (n_heads) *n_heads = 0;
  if (nc == 0) return 0;
  if (g_dead) return g_dead;
  const mh::Layout L = mh::layout((size_t)nc, (size_t)n_streams);
  const auto solve = [&](hipStream_t st, const void* carry, int ng, void* work) { return mh::launch_solve(st, carry, nc, ng, window, n_streams, work, L); };
  return call(words, nc, rx, n_streams, window, t_lo, t_hi, min_rx, mh::kMinRx, L, mlat_rule::parts(L, (size_t)nc, (size_t)n_streams), mh::launch_groups,
              solve, fixes, nullptr, 0, cap, n_fixes, member_stream, member_ts, member_cap, n_members, heads_out, n_heads);
}

// The emulator driver's entry point, argument for argument; -38: dev_mlat_set_carry was not called.
int sim_mlat(const double* ts, const unsigned char* bits14, const int* marker, const int* stream, int nc, const double* rx, int n_streams,
             double window, double t_lo, double t_hi, int min_rx, int grid, int zero_hash, void* fixes, int cap, int* n_fixes, int* member_stream,
             double* member_ts, int member_cap, int* n_members, int* heads_out, int* n_heads) {
  (void)grid;
  if (!g_carry) return -38;
  std::vector<unsigned long long> words((size_t)(nc > 0 ? nc : 0) * (mh::kEntBytes / 8) + 1, 0);
  if (nc > 0) g_carry(ts, bits14, marker, stream, nc, zero_hash, words.data());
  return dev_mlat_words(words.data(), nc, rx, n_streams, window, t_lo, t_hi, min_rx, fixes, cap, n_fixes, member_stream, member_ts, member_cap,
                        n_members, heads_out, n_heads);
}
}
