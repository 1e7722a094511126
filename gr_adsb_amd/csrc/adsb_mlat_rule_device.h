// adsb_mlat_rule_device.h -- device code of adsb_stream_mlat_rule's damped solver: THE DAMPED RULE of include/adsb_hip.h
// (MULTILATERATION), evaluated on adsb_mlat_device.h's device functions: the walk, the rows, the 4 x 4 step, the residual, the
// fix's address.  Everything in front of the solve -- the range, the heads, the compaction -- is adsb_mlat_device.h's; this header
// adds the two kernels that differ:
//
//   k_mlat_groups_rule  k_mlat_groups, but a group of exactly three used hearings whose head's payload gives no altitude gets
//                       nrx = 0, so that the compaction with min_w = 3 selects the three-hearing groups that can be solved and
//                       no others; selection, -ENOSPC and first[] come out of the compaction unchanged.
//   k_mlat_solve_lm     one wavefront per selected group, k_mlat_solve's walk, member lists and row; the solve is the damped
//                       run: per trial the 13 sums of J^T J and J^T r at the iterate and, unless the step is the untested last
//                       one, one sum of r^2 at the trial point (the residuals are recomputed for the trial, no second
//                       iterate is kept per lane), every lane factoring the
//                       same damped 4 x 4, so all lanes take every branch together -- the accept / reject decision, the end of
//                       a run, and whether a second run is made.  The altitude row is added by every lane from the same p, after
//                       the wave sums.  Lane 0 writes the fix and its Aux row.
//
// Every loop is bounded: the trials by kLmTrials, the runs by 2, the walk by the carry, the bit loop by 63, the broadcasts by
// 64.  No LDS.  All arithmetic in double; the height and the normal use sqrt and / only, so the emulator and the device agree
// bit for bit.  Device code only; needs adsb_mlat_device.h in front of it.
#pragma once

namespace adsb_mlat {

constexpr int kLmTrials = 64, kLmRuns = 2;
constexpr double kLmLambda0 = 1e-3, kLmLambdaMin = 1e-12, kLmLambdaMax = 1e12, kLmDown = 10.0, kLmUp = 10.0;
constexpr double kUpSecond = 30000.0;
constexpr int kRuleRestart = 1, kRuleAltitude = 2;                // ADSB_MLAT_RESTART, ADSB_MLAT_ALTITUDE
constexpr unsigned kAuxAided = 1u, kAuxRestarted = 2u, kAuxSecondKept = 4u;
constexpr double kWgsA = 6378137.0, kWgsF = 1.0 / 298.257223563, kWgsE2 = kWgsF * (2.0 - kWgsF), kWgsB = kWgsA * (1.0 - kWgsF);
constexpr double kWgsEp2 = kWgsE2 / (1.0 - kWgsE2), kFoot = 0.3048;

// adsb_mlat_aux
struct Aux {
  double up_m, lambda;
  int alt_ft, tries;
  unsigned flags;
  int reserved;
};

// The altitude the payload announces, in feet, or -1: the decoder's rule (dec_ac13 / dec_ac12 of adsb_device.h).  a: the
// reply's bytes 0 .. 7; every field used lies in them.
__device__ __forceinline__ int mlat_alt_ft(unsigned long long a) {
  const unsigned df = (unsigned)(a & 0xFFull) >> 3;
  const unsigned b2 = (unsigned)(a >> 16) & 0xFFu, b3 = (unsigned)(a >> 24) & 0xFFu, b4 = (unsigned)(a >> 32) & 0xFFu;
  const unsigned b5 = (unsigned)(a >> 40) & 0xFFu, b6 = (unsigned)(a >> 48) & 0xFFu;
  if (df == 0u || df == 4u || df == 16u || df == 20u) {
    const unsigned v = ((b2 & 0x1Fu) << 8) | b3;                  // bits 19 .. 31
    if (v == 0u || ((v >> 6) & 1u) || !((v >> 4) & 1u)) return -1;
    return (int)(((v >> 7) << 5) | (((v >> 5) & 1u) << 4) | (v & 0xFu)) * 25 - 1000;
  }
  if (df == 17u) {
    const unsigned tc = b4 >> 3;
    if (tc < 9u || tc > 18u) return -1;
    const unsigned v = (b5 << 4) | (b6 >> 4);                     // bits 40 .. 51
    if (!((v >> 4) & 1u)) return -1;
    return (int)(((v >> 5) << 4) | (v & 0xFu)) * 25 - 1000;
  }
  return -1;
}

// One Bowring step: the height of p above the ellipsoid and, when n is not null, the ellipsoid normal there.
__device__ __forceinline__ double mlat_height(double x, double y, double z, double* nx, double* ny, double* nz) {
  const double q = __builtin_sqrt(x * x + y * y);
  const double t = (z * kWgsA) / (q * kWgsB);                     // the tangent of the reduced latitude
  const double cb = 1.0 / __builtin_sqrt(1.0 + t * t), sb = t * cb;
  const double tp = (z + kWgsEp2 * kWgsB * (sb * sb * sb)) / (q - kWgsE2 * kWgsA * (cb * cb * cb));
  const double cp = 1.0 / __builtin_sqrt(1.0 + tp * tp), sp = tp * cp;
  if (nx) { *nx = cp * (x / q); *ny = cp * (y / q); *nz = sp; }
  return q * cp + z * sp - kWgsA * __builtin_sqrt(1.0 - kWgsE2 * (sp * sp));
}

// heads[n]: n = span[1] - span[0].  nrx[h] = the used hearings of head h's group; 0 for three of them without an altitude.
__global__ void __launch_bounds__(kThreads) k_mlat_groups_rule(const unsigned long long* carry, int nc, const int* heads, const int* span,
                                                               double window, const double* rx, int n_streams, int* nrx) {
  const int n = span[1] - span[0];
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  for (int h = (int)blockIdx.x * kWaves + wv; h < n; h += (int)gridDim.x * kWaves) {
    const int at = heads[h];
    if (at < 0 || at >= nc) { if (lane == 0) nrx[h] = 0; continue; }
    int k = mlat_group_used(carry, nc, at, window, lane, rx, n_streams);
    if (k == 3 && mlat_alt_ft(carry[(long long)at * kEntWords + 1]) == -1) k = 0;
    if (lane == 0) nrx[h] = k;
  }
}

// As k_mlat_solve; flags: kRuleRestart | kRuleAltitude; alt_weight: the altitude row's weight; aux[n].
__global__ void __launch_bounds__(kThreads) k_mlat_solve_lm(const unsigned long long* carry, int nc, const int* heads, const int* gsel, const int* gfirst,
                                                            const int* span, double window, const double* rx, int n_streams, int flags,
                                                            double alt_weight, Fix* fixes, Aux* aux, int* member_stream, double* member_ts) {
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
    const int alt_ft = (flags & kRuleAltitude) ? mlat_alt_ft(e[1]) : -1;
    const bool aided = alt_ft != -1;
    const double w = aided ? alt_weight : 0.0, h_want = kFoot * (double)alt_ft;
    // the centroid and the unit vector away from the Earth's centre; R_0 is the first used hearing's receiver
    const double cx = wave_sum(rxx) / nn, cy = wave_sum(rxy) / nn, cz = wave_sum(rxz) / nn;
    const double cn = __builtin_sqrt(cx * cx + cy * cy + cz * cz);
    const double vx = cx / cn, vy = cy / cn, vz = cz / cn;
    const int f = umask ? __builtin_ctzll(umask) : 0;
    const double r0x = __shfl(rxx, f), r0y = __shfl(rxy, f), r0z = __shfl(rxz, f);
    double sx = cx + kUp * vx, sy = cy + kUp * vy, sz = cz + kUp * vz;      // the run's start
    double kx = sx, ky = sy, kz = sz, kb = 0.0, klam = kLmLambda0, kup = 0.0;      // the kept run
    int kstatus = kNoConverge, kiters = 0, tries = 0;
    unsigned aflags = aided ? kAuxAided : 0u;
    for (int run = 0; run < kLmRuns; ++run) {         // (wave-uniform throughout: every lane holds the same sums)
      double px = sx, py = sy, pz = sz;
      const double hx = px - r0x, hy = py - r0y, hz = pz - r0z;
      double bb = __builtin_sqrt(hx * hx + hy * hy + hz * hz), lam = kLmLambda0;
      int status = kNoConverge, iters = 0;
      double S;
      {
        const double r = mlat_residual(H, px, py, pz, bb);
        const double ra = aided ? w * (mlat_height(px, py, pz, nullptr, nullptr, nullptr) - h_want) : 0.0;
        S = wave_sum(r * r) + ra * ra;
      }
      for (int trial = 0; trial < kLmTrials; ++trial) {
        const Row j = mlat_row(H, px, py, pz, bb);
        const double ux = j.ux, uy = j.uy, uz = j.uz, r = j.r;
        double jx = 0.0, jy = 0.0, jz = 0.0, ra = 0.0;             // the altitude row: w n(p), w (h(p) - h_want)
        if (aided) {
          double nx, ny, nz;
          const double h = mlat_height(px, py, pz, &nx, &ny, &nz);
          jx = w * nx; jy = w * ny; jz = w * nz; ra = w * (h - h_want);
        }
        const double mu = 1.0 + lam;
        const double a11 = (wave_sum(ux * ux) + jx * jx) * mu, a12 = wave_sum(ux * uy) + jx * jy, a13 = wave_sum(ux * uz) + jx * jz, a14 = wave_sum(-ux);
        const double a22 = (wave_sum(uy * uy) + jy * jy) * mu, a23 = wave_sum(uy * uz) + jy * jz, a24 = wave_sum(-uy);
        const double a33 = (wave_sum(uz * uz) + jz * jz) * mu, a34 = wave_sum(-uz), a44 = nn * mu;
        const double g1 = wave_sum(ux * r) + jx * ra, g2 = wave_sum(uy * r) + jy * ra, g3 = wave_sum(uz * r) + jz * ra, g4 = wave_sum(-r);
        const Step st = mlat_cholesky(a11, a12, a13, a14, a22, a23, a24, a33, a34, a44, g1, g2, g3, g4);
        if (!st.ok) { status = kSingular; break; }
        const double e1 = st.e1, e2 = st.e2, e3 = st.e3, e4 = st.e4;
        ++tries;
        const double qx = px + e1, qy = py + e2, qz = pz + e3, qb = bb + e4;      // the trial point
        const bool small = __builtin_sqrt(e1 * e1 + e2 * e2 + e3 * e3) < kStop;
        if (small && lam <= kLmLambda0) {             // the untested last step: rounding alone would decide S' <= S
          px = qx; py = qy; pz = qz; bb = qb;
          ++iters; status = kOk;
          break;
        }
        const double rt = mlat_residual(H, qx, qy, qz, qb);
        const double rat = aided ? w * (mlat_height(qx, qy, qz, nullptr, nullptr, nullptr) - h_want) : 0.0;
        const double S1 = wave_sum(rt * rt) + rat * rat;
        if (S1 <= 1.7976931348623157e308 && S1 <= S) {            // finite (a NaN compares false) and no worse: the step is taken
          px = qx; py = qy; pz = qz; bb = qb; S = S1;
          ++iters;
          lam = lam / kLmDown < kLmLambdaMin ? kLmLambdaMin : lam / kLmDown;
          if (small) { status = kOk; break; }
        } else {
          lam *= kLmUp;
          if (lam > kLmLambdaMax) break;              // (status is kNoConverge)
        }
      }
      const double up = (px - cx) * vx + (py - cy) * vy + (pz - cz) * vz;
      const bool good = status == kOk && up >= 0.0;
      if (run == 0 || good) { kx = px; ky = py; kz = pz; kb = bb; klam = lam; kup = up; kstatus = status; kiters = iters; }
      if (run == 0) {
        if (!(flags & kRuleRestart) || aided || good) break;
        aflags |= kAuxRestarted;
        if (status == kOk) { const double m = 2.0 * up; sx = px - m * vx; sy = py - m * vy; sz = pz - m * vz; }      // the mirror
        else { sx = cx + kUpSecond * vx; sy = cy + kUpSecond * vy; sz = cz + kUpSecond * vz; }
      } else if (good) {
        aflags |= kAuxSecondKept;
      }
    }
    const double rms = mlat_rms(mlat_residual(H, kx, ky, kz, kb), nn);      // the timing rows only
    if (lane == 0) {
      const unsigned long long a = e[1], b = e[2];
      const bool lng = (e[3] >> 56) == 2ull;
      Fix* o = fixes + g;
      o->ts = ts_h; o->x = kx; o->y = ky; o->z = kz; o->t_tx = ts_h - kb / kC; o->rms_m = rms;
      for (int k = 0; k < 8; ++k) o->bits[k] = (unsigned char)(a >> (8 * k));
      for (int k = 0; k < 6; ++k) o->bits[8 + k] = (unsigned char)(b >> (8 * k));
      o->flags = lng ? 64 : 0;
      o->icao = mlat_icao(a, b, lng);
      o->n_rx = n_rx; o->n_heard = n_heard; o->status = kstatus; o->iters = kiters; o->first = first;
      Aux* x = aux + g;
      x->up_m = kup; x->lambda = klam; x->alt_ft = alt_ft; x->tries = tries; x->flags = aflags; x->reserved = 0;
    }
  }
}

}  // namespace adsb_mlat
