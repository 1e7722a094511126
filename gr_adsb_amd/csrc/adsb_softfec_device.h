// adsb_softfec_device.h -- device code of the opt-in soft-decision CRC repair (ADSB_FLAG_FEC_SOFT; include/adsb_hip.h: SOFT
// REPAIR states the rule).  A parity failure of DF 11/17/18/19 that the Conservative table cannot explain is usually two to
// four wrong bits scattered over the reply, and the wrong bits are nearly always among the bits the slicer was least sure of:
// the samples behind every bit are still on the device, so the kernel ranks the bits by lo / hi of their two samples, keeps
// the n_weak weakest, and looks for the smallest subset of them whose syndromes XOR to the reply's.
//
//   k_soft_fec<MODE>    the delivered records of a pass, in place, behind k_fec (device list and pinned mirror)
//   k_soft_fec_slices   the slices of adsb_demod_work, behind k_fec_slices
//
// Cold code: only parity failures do work, nothing here is tuned.  One wavefront per record, grid-stride; a record that does
// not qualify leaves after one flag read.  Every kernel writes one 8-byte row (adsb_soft_fix) per record, zero for a record the
// rule does not apply to.  Plain C++ vector stores only.
//
// Device code only, as adsb_device.h: the includer provides the HIP device environment (adsb_wave_sync, adsb_wave_min_u32:
// adsb_env_hip.h, or the SIMT emulator of tests/sim).  The sample read, the CRC table, a record's syndrome and its pre-filter
// bits are adsb_reply_device.h's, shared with adsb_device.h.
#pragma once

#include "adsb_reply_device.h"

namespace adsb_softfec {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWeak = 16, kMaxFlips = 5;       // the caps of adsb_set_soft_fec
constexpr int kLaneBits = 6;                      // the masks are split over the 64 lanes by their top six bits
constexpr unsigned kNoMatch = 0xFFFFFFFFu;

struct Rule { int n_weak; int max_flips; float min_key; unsigned flags; };   // adsb_soft_fec_rule
static_assert(sizeof(Rule) == 16, "adsb_soft_fec_rule is 16 bytes");

// adsb_soft_fix as one little-endian word: nflip | ncand << 8 | bit[0..4] << 16.. | pad << 56
constexpr unsigned long long kRowNoBits = 0x00FFFFFFFFFF0000ull;
__device__ __forceinline__ unsigned long long row_make(int nflip, int ncand, unsigned long long fa, unsigned long long fb) {
  unsigned long long row = kRowNoBits | (unsigned long long)(unsigned)nflip | ((unsigned long long)(unsigned)ncand << 8);
#pragma unroll
  for (int q = 0; q < kMaxFlips; ++q) {
    int bit = -1;
    if (fa) { bit = __builtin_ctzll(fa); fa &= fa - 1; }
    else if (fb) { bit = 64 + __builtin_ctzll(fb); fb &= fb - 1; }
    if (bit >= 0) row = (row & ~(0xFFull << (16 + 8 * q))) | ((unsigned long long)(unsigned)bit << (16 + 8 * q));
  }
  return row;
}

// The weakness of a bit from its two samples: the slicer's own comparison picks hi and lo; one float32 division.
__device__ __forceinline__ float soft_key(float x1, float x0) {
  const float hi = x1 > x0 ? x1 : x0, lo = x1 > x0 ? x0 : x1;
  if (hi > 0.0f && lo >= 0.0f && hi < __builtin_inff()) return __fdiv_rn(lo, hi);
  return !(hi > 0.0f) ? 1.0f : 0.0f;
}

// message bits fa (0..63, bit = index) / fb (64..111) as the record words' bits: first bit = MSB of byte 0
__device__ __forceinline__ unsigned long long flip_word(unsigned long long f) { return __builtin_bswap64(__brevll(f)); }

// The rule for one qualifying reply (kDemod, DF 11/17/18/19, parity failed, no kFecDf: the caller's test), by a whole
// wavefront: w2 / w3 = its words (w3's flag bits are ignored and kept), p = the burst's local sample index, s_syn = 16 words
// of LDS of this wavefront.  On a match the bits are flipped in w2 / w3.  row = the record's adsb_soft_fix.  Wave-uniform.
template <int MODE>
__device__ __forceinline__ bool soft_repair(const void* data, long long n, float scale, int sps, long long p, unsigned long long& w2,
                                            unsigned long long& w3, const Rule& R, int lane, unsigned* s_syn, unsigned long long& row) {
  static constexpr adsb::CrcTab tab = adsb::make_crc_tab();
  const bool lng = ((1u << ((unsigned)(w2 & 0xFFu) >> 3)) & adsb::kDfLongSet) != 0;
  const int L = lng ? 112 : 56;
  const unsigned S = adsb::syndrome_of(w2, w3, lng ? 14 : 7);
  row = 0ull;
  if (S == 0u) return false;
  // 1. the keys of bits `lane` and `64 + lane`
  const int half = sps >> 1;
  const long long s0 = p + 8ll * sps + (long long)lane * sps;
  float k0 = 0.0f, k1 = 0.0f;
  if (lane < L) k0 = soft_key(adsb::xg<MODE>(data, n, s0, scale), adsb::xg<MODE>(data, n, s0 + half, scale));
  if (lng && lane < 48) {
    const long long s1 = s0 + 64ll * sps;
    k1 = soft_key(adsb::xg<MODE>(data, n, s1, scale), adsb::xg<MODE>(data, n, s1 + half, scale));
  }
  const bool v0 = lane >= 5 && lane < L && k0 >= R.min_key;
  const bool v1 = lng && lane < 48 && k1 >= R.min_key;
  const unsigned long long va = __ballot(v0), vb = __ballot(v1);
  // 2. ranks by broadcast comparisons: key descending, ties to the lower bit index
  int r0 = 0, r1 = 0;
  for (int j = 5; j < L; ++j) {
    if (!((j < 64 ? va >> j : vb >> (j - 64)) & 1ull)) continue;       // wave-uniform
    const float kj = __shfl(j < 64 ? k0 : k1, j & 63);
    r0 += (kj > k0 || (kj == k0 && j < lane)) ? 1 : 0;
    r1 += (kj > k1 || (kj == k1 && j < 64 + lane)) ? 1 : 0;
  }
  const int total = __popcll(va) + __popcll(vb);
  const int ncand = total < R.n_weak ? total : R.n_weak;
  row = row_make(0, ncand, 0ull, 0ull);
  if (ncand == 0) return false;
  const bool keep0 = v0 && r0 < ncand, keep1 = v1 && r1 < ncand;
  adsb_wave_sync();
  if (keep0) s_syn[r0] = tab.r[L - 1 - lane];
  if (keep1) s_syn[r1] = tab.r[L - 65 - lane];
  adsb_wave_sync();
  // 3. the 2^ncand masks: the lane is the top six bits, the rest is walked in Gray-code order
  const int low = ncand > kLaneBits ? ncand - kLaneBits : 0, top = ncand - low;
  unsigned best = kNoMatch;
  if (lane < (1 << top)) {
    unsigned s = 0u;
    for (int b = 0; b < top; ++b)
      if ((lane >> b) & 1) s ^= s_syn[low + b];
    const unsigned hi_mask = (unsigned)lane << low, steps = 1u << low;
    const int hi_pc = __builtin_popcount((unsigned)lane);
    unsigned g = 0u;
    for (unsigned t = 0u;;) {
      const unsigned mask = hi_mask | g;
      const int pc = hi_pc + __builtin_popcount(g);
      if (s == S && mask != 0u && pc <= R.max_flips) {
        const unsigned v = ((unsigned)pc << 16) | mask;
        best = v < best ? v : best;
      }
      if (++t == steps) break;
      const int b = __builtin_ctz(t);
      g ^= 1u << b;
      s ^= s_syn[b];
    }
  }
  // 4. fewest flips, then the smallest mask
  best = adsb_wave_min_u32(best);
  adsb_wave_sync();
  if (best == kNoMatch) return false;
  const unsigned mask = best & 0xFFFFu;
  const unsigned long long fa = __ballot(keep0 && ((mask >> (r0 & 15)) & 1u)), fb = __ballot(keep1 && ((mask >> (r1 & 15)) & 1u));
  w2 ^= flip_word(fa);
  w3 ^= flip_word(fb);
  row = row_make((int)(best >> 16), ncand, fa, fb);
  return true;
}

// the record's flags after a repair: the pre-filter bits recomputed as fec_record does, + kFecFixed
__device__ __forceinline__ unsigned repaired_flags(unsigned fl, unsigned long long a, unsigned long long b) {
  const unsigned keep = fl & ~(adsb::kParityOk | adsb::kLongFmt | adsb::kKnownDf | (31u << adsb::kDfShift));
  return keep | adsb::parity_flags_of(a, b) | adsb::kFecFixed;
}

// out: the pass's delivered list, four words per record, *n_kept of them (at most out_cap); host_out: the pinned mirror of
// the first host_cap records (may be null); rows[out_cap].  The samples: data / n / origin / scale / sps as k_confidence's.
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_soft_fec(const void* data, long long n, long long origin, float scale, int sps, Rule R,
                                                       unsigned long long* out, const int* n_kept, int out_cap,
                                                       unsigned long long* host_out, int host_cap, unsigned long long* rows) {
  __shared__ unsigned s_syn[kWaves][kMaxWeak];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int wave_g = (int)((blockIdx.x * (unsigned)kThreads + threadIdx.x) >> 6);
  const int nwave = (int)((gridDim.x * (unsigned)kThreads) >> 6);
  int nrec = *n_kept;
  if (nrec > out_cap) nrec = out_cap;
  for (int t = wave_g; t < nrec; t += nwave) {
    unsigned long long w3 = out[4ll * t + 3];
    const unsigned fl = (unsigned)(w3 >> 48);
    unsigned long long row = 0ull;
    if ((fl & adsb::kDemod) && !(fl & (adsb::kParityOk | adsb::kFecDf)) && ((1u << ((fl >> adsb::kDfShift) & 31u)) & adsb::kDfPiSet)) {
      unsigned long long w2 = out[4ll * t + 2];
      const long long p = (long long)out[4ll * t] - origin;
      if (soft_repair<MODE>(data, n, scale, sps, p, w2, w3, R, lane, s_syn[wave], row)) {
        w3 = (w3 & 0xFFFFFFFFFFFFull) | ((unsigned long long)repaired_flags(fl, w2, w3 & 0xFFFFFFFFFFFFull) << 48);
        if (lane == 0) {
          out[4ll * t + 2] = w2; out[4ll * t + 3] = w3;
          if (t < host_cap) { host_out[4ll * t + 2] = w2; host_out[4ll * t + 3] = w3; }
        }
      }
    }
    if (lane == 0) rows[t] = row;
  }
}

#ifndef ADSB_SOFTFEC_RULE_ONLY   // (adsb_softfec_batch_device.h takes the rule above and defines no second k_soft_fec_slices)
// The same for the stand-alone demod's slices: bits14 / ok as k_slice and k_fec_slices leave them (ok's bits 0, 5, 6, 7 = kDemod,
// kParityOk, kLongFmt, kKnownDf; bits 1 / 2 = kFecFixed / kFecDf >> 13), tag_idx[] local to the float chunk data[n].
__global__ void __launch_bounds__(kThreads) k_soft_fec_slices(const void* data, long long n, const long long* tag_idx, int sps, Rule R,
                                                              unsigned char* bits14, unsigned char* ok, int ntags, unsigned long long* rows) {
  __shared__ unsigned s_syn[kWaves][kMaxWeak];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int wave_g = (int)((blockIdx.x * (unsigned)kThreads + threadIdx.x) >> 6);
  const int nwave = (int)((gridDim.x * (unsigned)kThreads) >> 6);
  for (int t = wave_g; t < ntags; t += nwave) {
    const unsigned fl = ok[t];
    unsigned long long row = 0ull;
    if ((fl & adsb::kDemod) && !(fl & (adsb::kParityOk | (adsb::kFecDf >> 13)))) {
      unsigned char* q = bits14 + (long long)t * 14;
      unsigned long long w2 = 0ull, w3 = 0ull;
      for (int k = 0; k < 8; ++k) w2 |= (unsigned long long)q[k] << (8 * k);
      for (int k = 0; k < 6; ++k) w3 |= (unsigned long long)q[8 + k] << (8 * k);
      if (((1u << ((unsigned)(w2 & 0xFFu) >> 3)) & adsb::kDfPiSet) &&
          soft_repair<1>(data, n, 1.0f, sps, tag_idx[t], w2, w3, R, lane, s_syn[wave], row)) {
        const unsigned pf = adsb::parity_flags_of(w2, w3);
        if (lane == 0) {
          for (int k = 0; k < 8; ++k) q[k] = (unsigned char)(w2 >> (8 * k));
          for (int k = 0; k < 6; ++k) q[8 + k] = (unsigned char)(w3 >> (8 * k));
          ok[t] = (unsigned char)((fl & 1u) | (pf & 0xE0u) | (adsb::kFecFixed >> 13));
        }
      }
    }
    if (lane == 0) rows[t] = row;
  }
}

#endif  // ADSB_SOFTFEC_RULE_ONLY

}  // namespace adsb_softfec
