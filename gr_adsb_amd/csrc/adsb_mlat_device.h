// adsb_mlat_device.h -- device code of adsb_stream_mlat: the hearings of one reply that ADSB_FLAG_STREAM_DEDUP's carry holds,
// grouped and solved for the transmitter's position.  The group rule and the solver are stated once, in include/adsb_hip.h
// (MULTILATERATION); this header evaluates them.  The call reads the carry and writes buffers of its own: nothing of the
// decoder is touched.
//
// The launches of one call, on the carry c[0 .. nc) (adsb_dedup_device.h's entries: ts, payload a, b, hash | stream << 32 |
// marker << 56), in this order:
//
//   k_mlat_range    one thread: range = [first entry with ts >= t_lo, first entry with ts >= t_hi), by binary search on
//                   time_key.  Every later kernel reads the range from device memory, so nothing comes down for it.
//   k_mlat_heads    one thread per entry i of the range: w[i - lo] = 1 iff i is a HEAD -- marker != 0 and no entry q in front
//                   of it in carry order, from any stream, with an equal payload and ts[i] - ts[q] <= window.  k_dedup_find's
//                   scheme: a workgroup's 256 places share one superset range [q_lo, last), found by binary search with the
//                   rule's own test (monotone along the sorted carry), staged through LDS in tiles of kTile entries of 16 bytes
//                   (ts, hash | stream | marker); every thread reads the same staged element (a broadcast); time and the
//                   32-bit hash reject before the payload words are read from memory.  Thread i stops at its own place.
//   k_mlat_count    per chunk of 256 values: how many are >= min_w, and their sum  } the deterministic compaction: ballot
//   k_mlat_scan     one workgroup: both per-chunk arrays scanned in place, totals  } ranks, per-chunk counts, a scan.  No
//   k_mlat_place    per value >= min_w its rank: idx[rank] = its index (+ lo),      } output position is an atomic's return
//                   first[rank] = the sum of the taken values in front of it        } value.
//                   -> heads[0 .. nh) in carry order (min_w = 1; the sum is not used).  nh comes down.
//   k_mlat_groups   one wavefront per head: mlat_walk (below) -> nrx[h], the hearings the group would use.
//   k_mlat_count / _scan / _place over nrx[] with min_w = min_rx -> gsel[g] = h, first[g] = the scan of n_rx.  The group
//                   count and the member count come down; -ENOSPC is decided here.
//   k_mlat_solve    one wavefront per selected group: mlat_walk again (the members are cheaper to find twice than to keep for
//                   every head), lane k holding candidate k; the used lanes write member_stream / member_ts[first + rank];
//                   Gauss-Newton with the 13 sums of J^T J and J^T r reduced across the wavefront by an xor butterfly (a fixed
//                   order; every lane ends with the same bits, as IEEE addition commutes), every lane factoring the 4 x 4, all
//                   lanes leaving the loop together; lane 0 writes the fix.
//
// mlat_walk: the wavefront reads 64 entries behind the head at a time; a ballot marks those with ts - ts_head <= window and
// an equal payload; n_heard counts them all; the first 63 are lane-compacted behind the head (lane k takes the (k - cand)-th
// set bit of the ballot, by a shuffle); the walk ends with the first chunk that holds an entry outside the window or the
// carry's end.  The stream rule is at most 64 lane broadcasts.
//
// Every loop is bounded by the inputs: the binary searches by log2(nc), the scans and the walk by nc, the bit loop by 63,
// the broadcasts by 64, the solver by kMaxIter.  LDS: k_mlat_heads kHeadsLdsBytes, k_mlat_count / _place kPlaceLdsBytes,
// k_mlat_scan kScanLdsBytes, the others none.  Device code only; includes nothing.
// The device functions stand in front and the seven kernels behind them under one guard: with ADSB_MLAT_HELPERS_ONLY defined
// the kernels are left out.  adsb_mlat_rule.hip, the unit of adsb_stream_mlat_rule's kernels, walks, factors and names its
// fixes' addresses with the same functions and must not define these kernels a second time.
#pragma once

namespace adsb_mlat {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr int kEntWords = 4;
constexpr int kTile = 1024;                           // entries per LDS tile of k_mlat_heads: 16 bytes each
constexpr int kHeadsLdsBytes = kTile * 16 + 8;        // ... and the workgroup's range bound
constexpr int kPlaceLdsBytes = 2 * kWaves * 4;        // per wavefront a count and a sum
constexpr int kScanLdsBytes = 2 * kThreads * 4;
constexpr int kMaxCand = 64, kMaxIter = 32;
constexpr double kC = 299702547.0;                    // ADSB_MLAT_C
constexpr double kStop = 1e-3, kUp = 10000.0;
constexpr int kOk = 0, kNoConverge = 1, kSingular = 2;

// adsb_mlat_fix
struct Fix {
  double ts, x, y, z, t_tx, rms_m;
  unsigned char bits[14];
  unsigned short flags;
  int icao, n_rx, n_heard, status, iters, first;
};

// adsb_dedup_device.h's map: ascending keys <=> ascending doubles, -0.0 with +0.0
__device__ __forceinline__ unsigned long long time_key(double ts) {
  unsigned long long b = (unsigned long long)__double_as_longlong(ts);
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ent_ts(const unsigned long long* e, int i) { return __longlong_as_double((long long)e[(long long)i * kEntWords]); }
// THE test of the group rule, in double, with exactly this expression (later - earlier)
__device__ __forceinline__ bool in_window(double later, double earlier, double window) { return later - earlier <= window; }
// hash and marker (the length) equal; the streams may be anything
__device__ __forceinline__ bool meta_equal(unsigned long long m, unsigned long long mq) { return ((m ^ mq) & 0xFF000000FFFFFFFFull) == 0ull; }

// entries of c[0 .. nc) whose key is below key(t)
__device__ __forceinline__ int mlat_rank(const unsigned long long* c, int nc, double t) {
  const unsigned long long key = time_key(t);
  int lo = 0, hi = nc;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (time_key(ent_ts(c, mid)) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int wave_sum_int(int v) {
  for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// One wavefront, one head h.  Behind it lane k < cand holds candidate k of the head's group: its timestamp and stream (lane 0
// the head itself).  -> n_heard; *cand_out.  Called by all 64 lanes.
__device__ __forceinline__ int mlat_walk(const unsigned long long* carry, int nc, int h, double window, int lane, double* ts_out, int* stream_out,
                                         int* cand_out) {
  const unsigned long long* e = carry + (long long)h * kEntWords;
  const double ts_h = __longlong_as_double((long long)e[0]);
  const unsigned long long a = e[1], b = e[2], m = e[3];
  double ts_l = ts_h;
  int stream_l = (int)((m >> 32) & 0xFFFFFFull);
  int cand = 1, n_heard = 1;
  for (int base = h + 1; base < nc; base += kWave) {
    const int i = base + lane;
    bool in = false, match = false;
    double t = 0;
    int s = 0;
    if (i < nc) {
      const unsigned long long* q = carry + (long long)i * kEntWords;
      t = __longlong_as_double((long long)q[0]);
      in = in_window(t, ts_h, window);
      const unsigned long long mq = q[3];
      s = (int)((mq >> 32) & 0xFFFFFFull);
      match = in && meta_equal(m, mq) && q[1] == a && q[2] == b;
    }
    const unsigned long long inside = __ballot(in), mask = __ballot(match);
    const int hits = __popcll(mask);
    n_heard += hits;
    if (hits != 0 && cand < kMaxCand) {               // (wave-uniform)
      const int k = lane - cand;
      const bool want = k >= 0 && k < hits;
      unsigned long long mm = mask;
      if (want)
        for (int j = 0; j < k; ++j) mm &= mm - 1ull;  // the k-th set bit: at most 63 rounds
      const int src = want ? __builtin_ctzll(mm) : lane;
      const double t_src = __shfl(t, src);
      const int s_src = __shfl(s, src);
      if (want) { ts_l = t_src; stream_l = s_src; }
      cand = cand + hits < kMaxCand ? cand + hits : kMaxCand;
    }
    if (inside != ~0ull) break;                       // an entry outside the window, or the carry's end: the list is sorted
  }
  *ts_out = ts_l; *stream_out = stream_l; *cand_out = cand;
  return n_heard;
}

// Of the candidates, lane by lane: used iff the first of its stream and the stream has a position (rx[3 s] is not NaN).
__device__ __forceinline__ bool mlat_used(int lane, int cand, int stream, const double* rx, int n_streams) {
  bool used = lane < cand;
  for (int j = 0; j < cand; ++j) {                    // at most 64 broadcasts
    const int sj = __shfl(stream, j);
    if (j < lane && sj == stream) used = false;
  }
  if (used) {
    if ((unsigned)stream >= (unsigned)n_streams) used = false;
    else { const double x = rx[3ll * stream]; used = x == x; }
  }
  return used;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ bool pivot_ok(double d) { return d > 0.0 && d <= 1.7976931348623157e308; }

// The remainder of the reply's first nbits bits modulo x^24 + 0xFFF409: the address under address/parity.
__device__ __forceinline__ int mlat_remainder(unsigned long long a, unsigned long long b, int nbits) {
  unsigned v = 0;
  for (int i = 0; i < nbits; ++i) {
    const int byte = i >> 3;
    const unsigned by = (unsigned)((byte < 8 ? a >> (8 * byte) : b >> (8 * (byte - 8))) & 0xFFull);
    v = (v << 1) | ((by >> (7 - (i & 7))) & 1u);
    if (v & 0x1000000u) v ^= 0x1FFF409u;
  }
  return (int)v;
}

// ---- What k_mlat_solve and adsb_mlat_rule_device.h's k_mlat_solve_lm share.  The functions take and return values; every
// floating-point expression keeps its operand order (the tests compare bits).

// The used hearings of the group of the head at carry[at]: what both groups kernels count.
__device__ __forceinline__ int mlat_group_used(const unsigned long long* carry, int nc, int at, double window, int lane, const double* rx,
                                               int n_streams) {
  double ts; int stream, cand;
  (void)mlat_walk(carry, nc, at, window, lane, &ts, &stream, &cand);
  return __popcll(__ballot(mlat_used(lane, cand, stream, rx, n_streams)));
}

// One lane's hearing in a selected group: whether its candidate is used, that receiver's position (0 if not) and the range
// difference d = C (ts - ts_head).
struct Hearing {
  bool used;
  double rxx, rxy, rxz, d;
};

// The hearing's row of the Jacobian and its residual at the iterate (p, b): the unit vector from the receiver to p and
// rho - d - b; zeros for a lane that is not used.
struct Row { double ux, uy, uz, r; };
__device__ __forceinline__ Row mlat_row(const Hearing H, double px, double py, double pz, double bb) {
  const double dx = px - H.rxx, dy = py - H.rxy, dz = pz - H.rxz;
  const double rho = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
  Row j;
  j.ux = H.used ? dx / rho : 0.0; j.uy = H.used ? dy / rho : 0.0; j.uz = H.used ? dz / rho : 0.0;
  j.r = H.used ? rho - H.d - bb : 0.0;
  return j;
}

// The Cholesky factor of the symmetric 4 x 4 (a) and the step e that solves a e = -g; ok is false at the first pivot that is
// not positive and finite.
struct Step { double e1, e2, e3, e4; bool ok; };
__device__ __forceinline__ Step mlat_cholesky(double a11, double a12, double a13, double a14, double a22, double a23, double a24, double a33, double a34,
                                              double a44, double g1, double g2, double g3, double g4) {
  Step s = {0.0, 0.0, 0.0, 0.0, false};
  if (!pivot_ok(a11)) return s;
  const double l11 = __builtin_sqrt(a11), l21 = a12 / l11, l31 = a13 / l11, l41 = a14 / l11;
  const double d2 = a22 - l21 * l21;
  if (!pivot_ok(d2)) return s;
  const double l22 = __builtin_sqrt(d2), l32 = (a23 - l31 * l21) / l22, l42 = (a24 - l41 * l21) / l22;
  const double d3 = a33 - l31 * l31 - l32 * l32;
  if (!pivot_ok(d3)) return s;
  const double l33 = __builtin_sqrt(d3), l43 = (a34 - l41 * l31 - l42 * l32) / l33;
  const double d4 = a44 - l41 * l41 - l42 * l42 - l43 * l43;
  if (!pivot_ok(d4)) return s;
  const double l44 = __builtin_sqrt(d4);
  const double y1 = -g1 / l11, y2 = (-g2 - l21 * y1) / l22, y3 = (-g3 - l31 * y1 - l32 * y2) / l33;
  const double y4 = (-g4 - l41 * y1 - l42 * y2 - l43 * y3) / l44;
  s.e4 = y4 / l44; s.e3 = (y3 - l43 * s.e4) / l33; s.e2 = (y2 - l32 * s.e3 - l42 * s.e4) / l22;
  s.e1 = (y1 - l21 * s.e2 - l31 * s.e3 - l41 * s.e4) / l11;
  s.ok = true;
  return s;
}

// This lane's range residual at (p, b), 0 for a lane that is not used; and the rms of the group's residuals.
__device__ __forceinline__ double mlat_residual(const Hearing H, double px, double py, double pz, double bb) {
  const double fx = px - H.rxx, fy = py - H.rxy, fz = pz - H.rxz;
  return H.used ? __builtin_sqrt(fx * fx + fy * fy + fz * fz) - H.d - bb : 0.0;
}
__device__ __forceinline__ double mlat_rms(double rr, double nn) { return __builtin_sqrt(wave_sum(rr * rr) / nn); }

// The address a fix row states: the AA field of DF 11 / 17 / 18, the remainder under address/parity, else -1.  a, b: the
// reply's bytes 0 .. 7 and 8 .. 13; lng: 112 bits.
__device__ __forceinline__ int mlat_icao(unsigned long long a, unsigned long long b, bool lng) {
  const unsigned df = (unsigned)(a & 0xFFull) >> 3;
  const unsigned direct = (1u << 11) | (1u << 17) | (1u << 18), parity = (1u << 0) | (1u << 4) | (1u << 5) | (1u << 16) | (1u << 20) | (1u << 21);
  return ((1u << df) & direct) ? (int)((((a >> 8) & 0xFFull) << 16) | (((a >> 16) & 0xFFull) << 8) | ((a >> 24) & 0xFFull))
         : ((1u << df) & parity) ? mlat_remainder(a, b, lng ? 112 : 56) : -1;
}

#ifndef ADSB_MLAT_HELPERS_ONLY
__global__ void __launch_bounds__(kWave) k_mlat_range(const unsigned long long* carry, int nc, double t_lo, double t_hi, int* range) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int lo = mlat_rank(carry, nc, t_lo), hi = mlat_rank(carry, nc, t_hi);
  range[0] = lo;
  range[1] = hi < lo ? lo : hi;
}

// w[n]: n = range[1] - range[0]
__global__ void __launch_bounds__(kThreads) k_mlat_heads(const unsigned long long* carry, int nc, const int* range, double window, int* w) {
  __shared__ double tile_ts[kTile];
  __shared__ unsigned long long tile_meta[kTile];
  __shared__ int bound[2];
  const int i_lo = range[0], i_hi = range[1] < nc ? range[1] : nc;
  for (int base = i_lo + (int)blockIdx.x * kThreads; base < i_hi; base += (int)gridDim.x * kThreads) {
    const int i = base + (int)threadIdx.x;
    const int last = (base + kThreads < i_hi ? base + kThreads : i_hi) - 1;      // the workgroup's last place
    if (threadIdx.x == 0) {
      const double t0 = ent_ts(carry, base);
      int lo = 0, hi = base;                          // the first entry within the window of `base`
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (in_window(t0, ent_ts(carry, mid), window)) hi = mid; else lo = mid + 1; }
      bound[0] = lo;
    }
    __syncthreads();
    const int q_lo = bound[0];
    const bool live = i < i_hi;
    double ts = 0;
    unsigned long long a = 0, b = 0, m = 0;
    if (live) {
      const unsigned long long* e = carry + (long long)i * kEntWords;
      ts = __longlong_as_double((long long)e[0]); a = e[1]; b = e[2]; m = e[3];
    }
    const bool part = live && (m >> 56) != 0;
    bool found = false;                               // an equal payload in front of i, within the window
    for (int tb = q_lo; tb < last; tb += kTile) {
      const int cnt = last - tb < kTile ? last - tb : kTile;
      for (int j = (int)threadIdx.x; j < cnt; j += kThreads) {
        tile_ts[j] = ent_ts(carry, tb + j);
        tile_meta[j] = carry[(long long)(tb + j) * kEntWords + 3];
      }
      __syncthreads();
      if (part && !found) {
        const int stop = i - tb < cnt ? i - tb : cnt;
        for (int j = 0; j < stop; ++j) {
          if (!in_window(ts, tile_ts[j], window) || !meta_equal(m, tile_meta[j])) continue;
          const unsigned long long* q = carry + (long long)(tb + j) * kEntWords;
          if (q[1] == a && q[2] == b) { found = true; break; }
        }
      }
      __syncthreads();
    }
    if (live) w[i - i_lo] = part && !found ? 1 : 0;
    __syncthreads();                                  // bound[] is read by all and rewritten by thread 0 in the next round
  }
}

// span[0 .. 2): n = span[1] - span[0] values.  cnt[c] / sum[c]: of chunk c's 256 values, those >= min_w and their sum.
__global__ void __launch_bounds__(kThreads) k_mlat_count(const int* w, const int* span, int min_w, int* cnt, int* sum) {
  __shared__ int wave_cnt[kWaves], wave_sum[kWaves];
  const int n = span[1] - span[0], n_chunks = (n + kThreads - 1) / kThreads;
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
    const int i = c * kThreads + (int)threadIdx.x;
    const int v = i < n ? w[i] : 0;
    const bool take = v >= min_w;
    const int k = __popcll(__ballot(take)), s = wave_sum_int(take ? v : 0);
    if (lane == 0) { wave_cnt[wv] = k; wave_sum[wv] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int kk = 0, ss = 0;
      for (int q = 0; q < kWaves; ++q) { kk += wave_cnt[q]; ss += wave_sum[q]; }
      cnt[c] = kk; sum[c] = ss;
    }
    __syncthreads();
  }
}

// One workgroup: cnt[] and sum[] become their exclusive scans; tot = {0, the count, the sum, 0} ({tot[0], tot[1]} is the next
// compaction's span).
__global__ void __launch_bounds__(kThreads) k_mlat_scan(const int* span, int* cnt, int* sum, int* tot) {
  __shared__ int part_cnt[kThreads], part_sum[kThreads];
  if (blockIdx.x != 0) return;
  const int n = span[1] - span[0], n_chunks = (n + kThreads - 1) / kThreads;
  const int per = (n_chunks + kThreads - 1) / kThreads;
  const int lo = (int)threadIdx.x * per < n_chunks ? (int)threadIdx.x * per : n_chunks, hi = lo + per < n_chunks ? lo + per : n_chunks;
  int kk = 0, ss = 0;
  for (int c = lo; c < hi; ++c) { kk += cnt[c]; ss += sum[c]; }
  part_cnt[threadIdx.x] = kk; part_sum[threadIdx.x] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    int k0 = 0, s0 = 0;
    for (int t = 0; t < kThreads; ++t) {
      const int k1 = part_cnt[t], s1 = part_sum[t];
      part_cnt[t] = k0; part_sum[t] = s0;
      k0 += k1; s0 += s1;
    }
    tot[0] = 0; tot[1] = k0; tot[2] = s0; tot[3] = 0;
  }
  __syncthreads();
  kk = part_cnt[threadIdx.x]; ss = part_sum[threadIdx.x];
  for (int c = lo; c < hi; ++c) {
    const int k1 = cnt[c], s1 = sum[c];
    cnt[c] = kk; sum[c] = ss;
    kk += k1; ss += s1;
  }
}

// cnt[] / sum[]: k_mlat_scan's.  idx[rank] = the value's index (+ span[0] when add_lo); first[rank] (may be null) = the sum of
// the taken values in front of it.
__global__ void __launch_bounds__(kThreads) k_mlat_place(const int* w, const int* span, int min_w, const int* cnt, const int* sum, int add_lo,
                                                         int* idx, int* first) {
  __shared__ int wave_cnt[kWaves], wave_sum[kWaves];
  const int n = span[1] - span[0], n_chunks = (n + kThreads - 1) / kThreads;
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  const int add = add_lo ? span[0] : 0;
  for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
    const int i = c * kThreads + (int)threadIdx.x;
    const int v = i < n ? w[i] : 0;
    const bool take = v >= min_w;
    const unsigned long long mask = __ballot(take);
    int incl = take ? v : 0;                          // the wavefront's inclusive scan of the taken values
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(incl, (unsigned)d);
      if (lane >= d) incl += up;
    }
    if (lane == kWave - 1) { wave_cnt[wv] = __popcll(mask); wave_sum[wv] = incl; }
    __syncthreads();
    if (take) {
      int rank = cnt[c] + __popcll(mask & ((1ull << lane) - 1ull)), before = sum[c] + incl - v;
      for (int q = 0; q < wv; ++q) { rank += wave_cnt[q]; before += wave_sum[q]; }
      idx[rank] = i + add;
      if (first) first[rank] = before;
    }
    __syncthreads();
  }
}

// heads[n]: n = span[1] - span[0] (k_mlat_scan's totals).  nrx[h] = the used hearings of head h's group.
__global__ void __launch_bounds__(kThreads) k_mlat_groups(const unsigned long long* carry, int nc, const int* heads, const int* span, double window,
                                                          const double* rx, int n_streams, int* nrx) {
  const int n = span[1] - span[0];
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  for (int h = (int)blockIdx.x * kWaves + wv; h < n; h += (int)gridDim.x * kWaves) {
    const int at = heads[h];
    if (at < 0 || at >= nc) { if (lane == 0) nrx[h] = 0; continue; }
    const int k = mlat_group_used(carry, nc, at, window, lane, rx, n_streams);
    if (lane == 0) nrx[h] = k;
  }
}

// gsel[n] / gfirst[n]: n = span[1] - span[0]; heads[] as for k_mlat_groups.  fixes[n]; member_stream / member_ts at gfirst[g].
__global__ void __launch_bounds__(kThreads) k_mlat_solve(const unsigned long long* carry, int nc, const int* heads, const int* gsel, const int* gfirst,
                                                         const int* span, double window, const double* rx, int n_streams, Fix* fixes,
                                                         int* member_stream, double* member_ts) {
  const int n = span[1] - span[0];
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  for (int g = (int)blockIdx.x * kWaves + wv; g < n; g += (int)gridDim.x * kWaves) {
    const int at = heads[gsel[g]], first = gfirst[g];
    if (at < 0 || at >= nc) continue;
    double ts; int stream, cand;
    const int n_heard = mlat_walk(carry, nc, at, window, lane, &ts, &stream, &cand);
    const bool used = mlat_used(lane, cand, stream, rx, n_streams);
    const unsigned long long umask = __ballot(used);
    const int n_rx = __popcll(umask);
    if (used) {
      const int at_m = first + __popcll(umask & ((1ull << lane) - 1ull));
      member_stream[at_m] = stream; member_ts[at_m] = ts;
    }
    const unsigned long long* e = carry + (long long)at * kEntWords;
    const double ts_h = __longlong_as_double((long long)e[0]);
    const double rxx = used ? rx[3ll * stream] : 0.0, rxy = used ? rx[3ll * stream + 1] : 0.0, rxz = used ? rx[3ll * stream + 2] : 0.0;
    const double d = kC * (ts - ts_h);
    const Hearing H = {used, rxx, rxy, rxz, d};
    const double nn = (double)n_rx;
    // the start: the centroid, 10 km further from the Earth's centre; b0 from the first used hearing's receiver
    const double cx = wave_sum(rxx) / nn, cy = wave_sum(rxy) / nn, cz = wave_sum(rxz) / nn;
    const double cn = __builtin_sqrt(cx * cx + cy * cy + cz * cz);
    double px = cx + kUp * (cx / cn), py = cy + kUp * (cy / cn), pz = cz + kUp * (cz / cn);
    const int f = umask ? __builtin_ctzll(umask) : 0;
    const double hx = px - __shfl(rxx, f), hy = py - __shfl(rxy, f), hz = pz - __shfl(rxz, f);
    double bb = __builtin_sqrt(hx * hx + hy * hy + hz * hz);
    int status = kNoConverge, iters = 0;
    for (int it = 0; it < kMaxIter; ++it) {           // every lane holds the same sums: all leave together
      const Row j = mlat_row(H, px, py, pz, bb);
      const double a11 = wave_sum(j.ux * j.ux), a12 = wave_sum(j.ux * j.uy), a13 = wave_sum(j.ux * j.uz), a14 = wave_sum(-j.ux);
      const double a22 = wave_sum(j.uy * j.uy), a23 = wave_sum(j.uy * j.uz), a24 = wave_sum(-j.uy);
      const double a33 = wave_sum(j.uz * j.uz), a34 = wave_sum(-j.uz), a44 = nn;
      const double g1 = wave_sum(j.ux * j.r), g2 = wave_sum(j.uy * j.r), g3 = wave_sum(j.uz * j.r), g4 = wave_sum(-j.r);
      const Step s = mlat_cholesky(a11, a12, a13, a14, a22, a23, a24, a33, a34, a44, g1, g2, g3, g4);
      if (!s.ok) { status = kSingular; break; }
      px += s.e1; py += s.e2; pz += s.e3; bb += s.e4;
      ++iters;
      if (__builtin_sqrt(s.e1 * s.e1 + s.e2 * s.e2 + s.e3 * s.e3) < kStop) { status = kOk; break; }
    }
    const double rms = mlat_rms(mlat_residual(H, px, py, pz, bb), nn);
    if (lane == 0) {
      const unsigned long long a = e[1], b = e[2];
      const bool lng = (e[3] >> 56) == 2ull;
      Fix* o = fixes + g;
      o->ts = ts_h; o->x = px; o->y = py; o->z = pz; o->t_tx = ts_h - bb / kC; o->rms_m = rms;
      for (int k = 0; k < 8; ++k) o->bits[k] = (unsigned char)(a >> (8 * k));
      for (int k = 0; k < 6; ++k) o->bits[8 + k] = (unsigned char)(b >> (8 * k));
      o->flags = lng ? 64 : 0;
      o->icao = mlat_icao(a, b, lng);
      o->n_rx = n_rx; o->n_heard = n_heard; o->status = status; o->iters = iters; o->first = first;
    }
  }
}
#endif  // ADSB_MLAT_HELPERS_ONLY

}  // namespace adsb_mlat
