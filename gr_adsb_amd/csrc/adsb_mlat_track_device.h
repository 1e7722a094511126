// adsb_mlat_track_device.h -- device code of adsb_stream_mlat_track and the store's readout and expiry: the fixes of one
// multilateration call, fused per 24-bit address into a store of tracks that stays on the device.  The rule is stated once, in
// include/adsb_hip.h (MLAT TRACKS); this header evaluates it.  The call reads the fixes and aux rows the solve kernels left in
// their work buffer and the store, and writes the store's other buffer: nothing of the decoder or the carry is touched.
//
// The store is rows[0 .. nt) of 96 bytes (adsb_mlat_track) in ascending icao, each address once.  It is a sorted array and not
// a hash table: no row is ever the target of an atomic, a row's place is a function of the addresses alone, so the same calls
// give the same bytes, and the readout is in order as it lies.
//
// The launches of one update, on fixes[0 .. ng):
//
//   k_track_eligible  w[i] = 1 iff fixes[i].icao >= 0; clears the call's totals
//   k_track_count / _scan / _place   the deterministic compaction of adsb_mlat_device.h (256-entry chunks, ballot ranks, a scan):
//                     sel[0 .. nk) = the eligible rows in row order.  nk comes down: the sort's size is the host's.
//   k_track_keys      keys[r] = icao << 32 | row, vals[r] = row
//   (adsb_shared.h's launch_sort: the stable 64-bit key sort, 4096-key tiles)  -> ascending (icao, row): each address's fixes
//                     lie together, in row order, which is carry order, which is ascending ts
//   k_track_heads     w[r] = 1 iff r is the first key of its address's run; compaction -> run_start[0 .. nr)
//   k_track_find      one lane per run: its length; pos = the old rows with a smaller address (binary search); w[j] = 1 iff the
//                     address is NEW -- not in the old store -- and one of its fixes is USABLE, so that a row it is given is
//                     never left empty; compaction -> newidx[0 .. n_new), in address order
//   k_track_move      one thread per word of an old row: to index + (new addresses below it), by binary search over the new list
//   k_track_update    one lane per run: the row -- the old one, or none -- through steps 1 to 5 for each of the run's fixes in
//                     order, then written at pos + (new addresses below it); of a fix the lane reads five doubles and two ints,
//                     and up_m of its aux row.  The call's totals are integer atomics after a wavefront reduction.
//
// Readout and expiry: k_track_pick (w[i] = n_fixes >= min_fixes and last_ts >= cutoff), the compaction, k_track_gather (the rows'
// words to their ranks in the other buffer).
//
// Every loop is bounded by the inputs: the grid-stride loops by their counts, the binary searches by log2, the walk of a run by
// its length.  LDS: k_track_count / _place kPlaceLdsBytes, k_track_scan kScanLdsBytes, the others none.  Device code only;
// includes nothing.
#pragma once

namespace adsb_mlat_track {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr int kPlaceLdsBytes = kWaves * 4, kScanLdsBytes = kThreads * 4;
constexpr int kRowWords = 12;                         // a track row as 64-bit words
constexpr int kOk = 0;                                // ADSB_MLAT_OK
constexpr unsigned kGap = 1u, kRestarted = 2u;        // ADSB_TRACK_GAP, ADSB_TRACK_RESTARTED
// the call's totals: words of stats[]
constexpr int kUnusable = 0, kStale = 1, kRejected = 2, kTaken = 3, kStarted = 4, kStatWords = 8;
// cnts[]: the counts the kernels hand on to each other and to the host
constexpr int kCntIn = 0, kCntKeys = 1, kCntRuns = 2, kCntNew = 3, kCntWords = 16;

// adsb_mlat_fix, adsb_mlat_aux, adsb_mlat_track_rule, adsb_mlat_track
struct Fix {
  double ts, x, y, z, t_tx, rms_m;
  unsigned char bits[14];
  unsigned short flags;
  int icao, n_rx, n_heard, status, iters, first;
};
struct Aux { double up_m, lambda; int alt_ft, tries; unsigned flags; int reserved; };
struct Rule {
  double alpha, beta, gate_m, max_speed_mps, max_gap_s, max_rms_m, min_up_m;
  int restart_after, reserved;
};
struct Track {
  int icao; unsigned flags; int n_fixes, n_rejected;
  double first_ts, last_ts, x, y, z, vx, vy, vz, rms_m;
  int n_rx, misses;
};

__device__ __forceinline__ bool track_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

// Step 1 of the rule.  aux may be null (ADSB_MLAT_SOLVER_GN: up_m is 0).
__device__ __forceinline__ bool track_usable(const Fix* f, const Aux* aux, int row, const Rule& R) {
  const double up = aux ? aux[row].up_m : 0.0, rms = f->rms_m;
  return f->status == kOk && track_finite(f->x) && track_finite(f->y) && track_finite(f->z) && track_finite(rms) && rms <= R.max_rms_m &&
         up >= R.min_up_m;
}

__device__ __forceinline__ int key_icao(unsigned long long key) { return (int)(key >> 32); }
__device__ __forceinline__ int key_row(unsigned long long key) { return (int)(key & 0xFFFFFFFFull); }

// the new addresses below icao: newidx[0 .. n_new) names the runs of the new addresses, ascending
__device__ __forceinline__ int new_below(const unsigned long long* keys, const int* run_start, const int* newidx, int n_new, int icao) {
  int lo = 0, hi = n_new;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key_icao(keys[run_start[newidx[mid]]]) < icao) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
  for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// The start of a track at fix values (step 3, and step 4's restart): flags and n_rejected are the caller's to keep.
__device__ __forceinline__ void track_start(Track& T, double ts, double x, double y, double z, double rms, int n_rx) {
  T.x = x; T.y = y; T.z = z; T.vx = 0.0; T.vy = 0.0; T.vz = 0.0;
  T.first_ts = ts; T.last_ts = ts; T.n_fixes = 1; T.misses = 0; T.rms_m = rms; T.n_rx = n_rx;
}

__global__ void __launch_bounds__(kThreads) k_track_eligible(const Fix* fixes, int n, int* w, int* cnts, unsigned long long* stats) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cnts[kCntIn] = n; cnts[kCntKeys] = 0; cnts[kCntRuns] = 0; cnts[kCntNew] = 0;
    for (int k = 0; k < kStatWords; ++k) stats[k] = 0ull;
  }
  for (int i = (int)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int)gridDim.x * kThreads) w[i] = fixes[i].icao >= 0 ? 1 : 0;
}

// w[*np] -> cnt[c]: the set flags of chunk c's 256
__global__ void __launch_bounds__(kThreads) k_track_count(const int* w, const int* np, int* cnt) {
  __shared__ int wave_cnt[kWaves];
  const int n = *np, n_chunks = (n + kThreads - 1) / kThreads;
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
    const int i = c * kThreads + (int)threadIdx.x;
    const int k = __popcll(__ballot(i < n && w[i] != 0));
    if (lane == 0) wave_cnt[wv] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
      int kk = 0;
      for (int q = 0; q < kWaves; ++q) kk += wave_cnt[q];
      cnt[c] = kk;
    }
    __syncthreads();
  }
}

// One workgroup: cnt[] becomes its exclusive scan; *tot = the number of set flags.
__global__ void __launch_bounds__(kThreads) k_track_scan(const int* np, int* cnt, int* tot) {
  __shared__ int part_cnt[kThreads];
  if (blockIdx.x != 0) return;
  const int n = *np, n_chunks = (n + kThreads - 1) / kThreads;
  const int per = (n_chunks + kThreads - 1) / kThreads;
  const int lo = (int)threadIdx.x * per < n_chunks ? (int)threadIdx.x * per : n_chunks, hi = lo + per < n_chunks ? lo + per : n_chunks;
  int kk = 0;
  for (int c = lo; c < hi; ++c) kk += cnt[c];
  part_cnt[threadIdx.x] = kk;
  __syncthreads();
  if (threadIdx.x == 0) {
    int k0 = 0;
    for (int t = 0; t < kThreads; ++t) { const int k1 = part_cnt[t]; part_cnt[t] = k0; k0 += k1; }
    *tot = k0;
  }
  __syncthreads();
  kk = part_cnt[threadIdx.x];
  for (int c = lo; c < hi; ++c) { const int k1 = cnt[c]; cnt[c] = kk; kk += k1; }
}

// cnt[]: k_track_scan's.  idx[rank] = the index of the rank-th set flag.
__global__ void __launch_bounds__(kThreads) k_track_place(const int* w, const int* np, const int* cnt, int* idx) {
  __shared__ int wave_cnt[kWaves];
  const int n = *np, n_chunks = (n + kThreads - 1) / kThreads;
  const int lane = (int)threadIdx.x & (kWave - 1), wv = (int)threadIdx.x / kWave;
  for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
    const int i = c * kThreads + (int)threadIdx.x;
    const bool take = i < n && w[i] != 0;
    const unsigned long long mask = __ballot(take);
    if (lane == 0) wave_cnt[wv] = __popcll(mask);
    __syncthreads();
    if (take) {
      int rank = cnt[c] + __popcll(mask & ((1ull << lane) - 1ull));
      for (int q = 0; q < wv; ++q) rank += wave_cnt[q];
      idx[rank] = i;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads) k_track_keys(const Fix* fixes, const int* sel, const int* np, unsigned long long* keys, unsigned* vals) {
  const int n = *np;
  for (int r = (int)blockIdx.x * kThreads + (int)threadIdx.x; r < n; r += (int)gridDim.x * kThreads) {
    const int row = sel[r];
    keys[r] = ((unsigned long long)(unsigned)fixes[row].icao << 32) | (unsigned long long)(unsigned)row;
    vals[r] = (unsigned)row;
  }
}

__global__ void __launch_bounds__(kThreads) k_track_heads(const unsigned long long* keys, const int* np, int* w) {
  const int n = *np;
  for (int r = (int)blockIdx.x * kThreads + (int)threadIdx.x; r < n; r += (int)gridDim.x * kThreads)
    w[r] = r == 0 || key_icao(keys[r]) != key_icao(keys[r - 1]) ? 1 : 0;
}

// run_start[*n_runs]; keys[*n_keys].  old[nt]: the store.
__global__ void __launch_bounds__(kThreads) k_track_find(const unsigned long long* keys, const int* run_start, const int* n_runs, const int* n_keys,
                                                         const Fix* fixes, const Aux* aux, Rule R, const Track* old, int nt, int* run_len, int* pos,
                                                         int* w) {
  const int n = *n_runs, nk = *n_keys;
  for (int j = (int)blockIdx.x * kThreads + (int)threadIdx.x; j < n; j += (int)gridDim.x * kThreads) {
    const int at = run_start[j], len = (j + 1 < n ? run_start[j + 1] : nk) - at;
    const int icao = key_icao(keys[at]);
    int lo = 0, hi = nt;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (old[mid].icao < icao) lo = mid + 1; else hi = mid;
    }
    bool fresh = !(lo < nt && old[lo].icao == icao), usable = false;
    if (fresh)
      for (int k = 0; k < len && !usable; ++k) {
        const int row = key_row(keys[at + k]);
        usable = track_usable(fixes + row, aux, row, R);
      }
    run_len[j] = len; pos[j] = lo; w[j] = fresh && usable ? 1 : 0;
  }
}

// next[i + (new addresses below old[i])] = old[i], word by word
__global__ void __launch_bounds__(kThreads) k_track_move(const Track* old, int nt, const unsigned long long* keys, const int* run_start,
                                                         const int* newidx, const int* n_new, Track* next) {
  const long long total = (long long)nt * kRowWords;
  const int nn = *n_new;
  const unsigned long long* src = (const unsigned long long*)old;
  unsigned long long* dst = (unsigned long long*)next;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long long)gridDim.x * kThreads) {
    const int i = (int)(t / kRowWords), word = (int)(t % kRowWords);
    const int to = i + new_below(keys, run_start, newidx, nn, old[i].icao);
    dst[(long long)to * kRowWords + word] = src[t];
  }
}

// One lane per run.  next[]: k_track_move's; a run's row is written whole, or -- when no track exists at the run's end -- not at all.
__global__ void __launch_bounds__(kThreads) k_track_update(const unsigned long long* keys, const int* run_start, const int* run_len, const int* pos,
                                                           const int* n_runs, const int* newidx, const int* n_new, const Fix* fixes, const Aux* aux,
                                                           Rule R, const Track* old, int nt, Track* next, unsigned long long* stats) {
  const int n = *n_runs, nn = *n_new;
  long long s_unusable = 0, s_stale = 0, s_rejected = 0, s_taken = 0, s_started = 0;
  for (int j = (int)blockIdx.x * kThreads + (int)threadIdx.x; j < n; j += (int)gridDim.x * kThreads) {
    const int at = run_start[j], len = run_len[j], lo = pos[j];
    const int icao = key_icao(keys[at]);
    Track T;
    bool exists = lo < nt && old[lo].icao == icao;
    if (exists) T = old[lo];
    else { T.icao = icao; T.flags = 0u; T.n_fixes = 0; T.n_rejected = 0; track_start(T, 0.0, 0.0, 0.0, 0.0, 0.0, 0); }
    for (int k = 0; k < len; ++k) {
      const int row = key_row(keys[at + k]);
      const Fix* f = fixes + row;
      if (!track_usable(f, aux, row, R)) { ++s_unusable; continue; }                       // 1. USABLE
      const double ts = f->ts, fx = f->x, fy = f->y, fz = f->z;
      if (exists && ts <= T.last_ts) { ++s_stale; continue; }                              // 2. STALE
      if (!exists || ts - T.last_ts > R.max_gap_s) {                                       // 3. START
        if (exists) T.flags |= kGap;
        track_start(T, ts, fx, fy, fz, f->rms_m, f->n_rx);
        exists = true; ++s_started;
        continue;
      }
      const double dt = ts - T.last_ts;                                                    // 4. GATE
      const double ppx = T.x + T.vx * dt, ppy = T.y + T.vy * dt, ppz = T.z + T.vz * dt;
      const double dx = fx - ppx, dy = fy - ppy, dz = fz - ppz;
      const double dist = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
      if (dist > R.gate_m + R.max_speed_mps * dt) {
        ++T.n_rejected; ++T.misses; ++s_rejected;
        if (T.misses >= R.restart_after) {
          T.flags |= kRestarted;
          track_start(T, ts, fx, fy, fz, f->rms_m, f->n_rx);
          ++s_started;
        }
        continue;
      }
      const double gv = R.beta / dt;                                                       // 5. STEP
      T.x = ppx + R.alpha * dx; T.y = ppy + R.alpha * dy; T.z = ppz + R.alpha * dz;
      T.vx = T.vx + gv * dx; T.vy = T.vy + gv * dy; T.vz = T.vz + gv * dz;
      T.last_ts = ts; T.n_fixes += 1; T.misses = 0; T.rms_m = f->rms_m; T.n_rx = f->n_rx;
      ++s_taken;
    }
    if (exists) next[lo + new_below(keys, run_start, newidx, nn, icao)] = T;
  }
  s_unusable = wave_sum_ll(s_unusable); s_stale = wave_sum_ll(s_stale); s_rejected = wave_sum_ll(s_rejected);
  s_taken = wave_sum_ll(s_taken); s_started = wave_sum_ll(s_started);
  if (((int)threadIdx.x & (kWave - 1)) == 0) {
    if (s_unusable) atomicAdd(&stats[kUnusable], (unsigned long long)s_unusable);
    if (s_stale) atomicAdd(&stats[kStale], (unsigned long long)s_stale);
    if (s_rejected) atomicAdd(&stats[kRejected], (unsigned long long)s_rejected);
    if (s_taken) atomicAdd(&stats[kTaken], (unsigned long long)s_taken);
    if (s_started) atomicAdd(&stats[kStarted], (unsigned long long)s_started);
  }
}

// w[i] = 1 iff rows[i] is asked for; cnts[kCntIn] = n
__global__ void __launch_bounds__(kThreads) k_track_pick(const Track* rows, int n, int min_fixes, double cutoff, int* w, int* cnts) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { cnts[kCntIn] = n; cnts[kCntKeys] = 0; }
  for (int i = (int)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int)gridDim.x * kThreads)
    w[i] = rows[i].n_fixes >= min_fixes && rows[i].last_ts >= cutoff ? 1 : 0;
}

// out[r] = rows[idx[r]], word by word
__global__ void __launch_bounds__(kThreads) k_track_gather(const Track* rows, const int* idx, const int* np, Track* out) {
  const long long total = (long long)*np * kRowWords;
  const unsigned long long* src = (const unsigned long long*)rows;
  unsigned long long* dst = (unsigned long long*)out;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long long)gridDim.x * kThreads)
    dst[t] = src[(long long)idx[t / kRowWords] * kRowWords + t % kRowWords];
}

}  // namespace adsb_mlat_track
