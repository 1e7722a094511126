// adsb_softfec.hip -- the translation unit of the soft-decision CRC repair's kernels (adsb_softfec_device.h), their launchers
// (adsb_softfec.h) and the rule as plain host arithmetic (adsb_mode_s_soft_fec).  A seventh unit, so that the kernels of the
// other six and their resource reports are exactly what they are without it.  Linked into libadsb_hip.so.
#include <hip/hip_runtime.h>

#include <string.h>

#if defined(__HIP__)
#include "adsb_env_hip.h"
#endif   // (a host compiler gets the SIMT emulator's environment with its <hip/hip_runtime.h>: tools/softfec_sanitize.sh)
#include "adsb_softfec.h"
#include "adsb_softfec_device.h"
#include "../../include/adsb_hip.h"

namespace adsb_softfec_host {

using namespace adsb_softfec;

static_assert(kRowBytes == sizeof(adsb_soft_fix) && kRuleBytes == sizeof(Rule) && sizeof(adsb_soft_fec_rule) == sizeof(Rule) &&
              kWavesPerGroup == kWaves, "the header's sizes are the device code's");
static_assert(offsetof(adsb_soft_fix, ncand) == 1 && offsetof(adsb_soft_fix, bit) == 2 && offsetof(adsb_soft_fix, pad) == 7 &&
              offsetof(adsb_soft_fec_rule, max_flips) == offsetof(Rule, max_flips) && offsetof(adsb_soft_fec_rule, min_key) == offsetof(Rule, min_key),
              "a row is one little-endian word; the rule's fields are the device's");
static_assert(adsb::kDemod == ADSB_BURST_DEMOD && adsb::kParityOk == ADSB_BURST_PARITY_OK && adsb::kFecFixed == ADSB_BURST_FEC_FIXED &&
              adsb::kFecDf == ADSB_BURST_FEC_DF, "the record flags are the ABI's");

namespace {
template <int MODE>
void launch_mode(hipStream_t st, unsigned grid, const void* data, long long n, long long origin, float scale, int sps, const Rule& R,
                 unsigned long long* out, const int* n_kept, int out_cap, unsigned long long* host_out, int host_cap, unsigned long long* rows) {
  hipLaunchKernelGGL((k_soft_fec<MODE>), dim3(grid), dim3(kThreads), 0, st, data, n, origin, scale, sps, R, out, n_kept, out_cap, host_out,
                     host_cap, rows);
}
}  // namespace

int launch_records(void* stream, unsigned grid, int mode, const void* data, long long n, long long origin, float scale, int sps,
                   const void* rule, void* out, const int* n_kept, int out_cap, void* host_out, int host_cap, void* rows) {
  if (out_cap <= 0 || grid == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  Rule R;
  memcpy(&R, rule, sizeof R);
  unsigned long long* const o = (unsigned long long*)out;
  unsigned long long* const h = (unsigned long long*)host_out;
  unsigned long long* const r = (unsigned long long*)rows;
  switch (mode) {
    case 0: launch_mode<0>(st, grid, data, n, origin, scale, sps, R, o, n_kept, out_cap, h, h ? host_cap : 0, r); break;
    case 1: launch_mode<1>(st, grid, data, n, origin, scale, sps, R, o, n_kept, out_cap, h, h ? host_cap : 0, r); break;
    case 2: launch_mode<2>(st, grid, data, n, origin, scale, sps, R, o, n_kept, out_cap, h, h ? host_cap : 0, r); break;
    case 3: launch_mode<3>(st, grid, data, n, origin, scale, sps, R, o, n_kept, out_cap, h, h ? host_cap : 0, r); break;
    case 4: launch_mode<4>(st, grid, data, n, origin, scale, sps, R, o, n_kept, out_cap, h, h ? host_cap : 0, r); break;
    default: return 1;   // hipErrorInvalidValue
  }
  return (int)hipGetLastError();
}

int launch_slices(void* stream, unsigned grid, const void* data, long long n, const long long* tag_idx, int sps, const void* rule,
                  unsigned char* bits14, unsigned char* ok, int ntags, void* rows) {
  if (ntags <= 0 || grid == 0) return 0;
  Rule R;
  memcpy(&R, rule, sizeof R);
  hipLaunchKernelGGL(k_soft_fec_slices, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, data, n, tag_idx, sps, R, bits14, ok, ntags,
                     (unsigned long long*)rows);
  return (int)hipGetLastError();
}

}  // namespace adsb_softfec_host

// ---- the rule as plain host arithmetic (include/adsb_hip.h: SOFT REPAIR) ----------------------------------------------------
namespace {
inline int host_bit(const uint8_t* b, int i) { return (b[i >> 3] >> (7 - (i & 7))) & 1; }
// pre-filter flags of one payload and its syndrome for the DF's own length
uint32_t host_flags(const uint8_t b[14], uint32_t* syn_out, int* L_out) {
  static constexpr adsb::CrcTab tab = adsb::make_crc_tab();
  const unsigned df = b[0] >> 3, dfb = 1u << df;
  const bool lng = (dfb & adsb::kDfLongSet) != 0, known = lng || (dfb & adsb::kDfShortSet) != 0;
  const int L = lng ? 112 : 56;
  uint32_t syn = 0;
  for (int i = 0; i < L; ++i)
    if (host_bit(b, i)) syn ^= tab.r[L - 1 - i];
  uint32_t f = (uint32_t)df << ADSB_BURST_DF_SHIFT;
  if (lng) f |= ADSB_BURST_LONG;
  if (known) f |= ADSB_BURST_KNOWN_DF;
  if ((dfb & adsb::kDfPiSet) && syn == 0) f |= ADSB_BURST_PARITY_OK;
  if (syn_out) *syn_out = syn;
  if (L_out) *L_out = L;
  return f;
}
}  // namespace

extern "C" uint32_t adsb_mode_s_soft_fec(const uint8_t in[14], const float key[112], const adsb_soft_fec_rule* rule, uint8_t out[14],
                                         adsb_soft_fix* fix) {
  static constexpr adsb::CrcTab tab = adsb::make_crc_tab();
  const adsb_soft_fec_rule R = rule ? *rule : adsb_soft_fec_rule{8, 3, 0.0f, 0u};
  uint8_t b[14];
  memcpy(b, in, 14);
  if (out) memcpy(out, b, 14);
  adsb_soft_fix row;
  memset(&row, 0, sizeof row);
  if (fix) *fix = row;
  uint32_t S = 0;
  int L = 0;
  const uint32_t flags = host_flags(b, &S, &L);
  if (!key || !((1u << (b[0] >> 3)) & adsb::kDfPiSet) || S == 0) return flags;
  // candidates: bits 5 .. L-1 with key >= min_key, key descending, ties to the lower index; the first n_weak
  int cand[112], nc = 0;
  for (int i = 5; i < L; ++i)
    if (key[i] >= R.min_key) cand[nc++] = i;
  for (int i = 1; i < nc; ++i)
    for (int k = i; k > 0 && key[cand[k - 1]] < key[cand[k]]; --k) { const int t = cand[k]; cand[k] = cand[k - 1]; cand[k - 1] = t; }
  const int n_weak = R.n_weak < 1 ? 1 : R.n_weak > adsb_softfec::kMaxWeak ? adsb_softfec::kMaxWeak : R.n_weak;
  const int max_flips = R.max_flips > adsb_softfec::kMaxFlips ? adsb_softfec::kMaxFlips : R.max_flips;   // (a row names five bits)
  if (nc > n_weak) nc = n_weak;
  row.ncand = (uint8_t)nc;
  memset(row.bit, 0xFF, sizeof row.bit);
  uint32_t best = adsb_softfec::kNoMatch;
  for (uint32_t mask = 1; mask < (1u << nc); ++mask) {
    const int pc = __builtin_popcount(mask);
    if (pc > max_flips) continue;
    uint32_t s = 0;
    for (int k = 0; k < nc; ++k)
      if ((mask >> k) & 1u) s ^= tab.r[L - 1 - cand[k]];
    if (s != S) continue;
    const uint32_t v = ((uint32_t)pc << 16) | mask;
    if (v < best) best = v;
  }
  if (best == adsb_softfec::kNoMatch) { if (fix) *fix = row; return flags; }
  bool flip[112] = {false};
  for (int k = 0; k < nc; ++k)
    if ((best >> k) & 1u) flip[cand[k]] = true;
  int q = 0;
  for (int i = 0; i < L; ++i)
    if (flip[i]) { b[i >> 3] ^= (uint8_t)(0x80u >> (i & 7)); row.bit[q++] = (uint8_t)i; }
  row.nflip = (uint8_t)q;
  if (out) memcpy(out, b, 14);
  if (fix) *fix = row;
  return host_flags(b, nullptr, nullptr) | ADSB_BURST_FEC_FIXED;
}
