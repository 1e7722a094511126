// adsb_dedup_device.h -- device code of ADSB_FLAG_STREAM_DEDUP: replies heard by several receivers of a shared decoder are
// published once.  The rule is stated once, in include/adsb_hip.h (DE-DUPLICATION); this header evaluates it.
//
// The step sits in fleet_step between k_shared_gather and k_fleet_announce, on the call's time-ordered list, and once more
// behind k_shared_scatter:
//
//   k_dedup_entries   per place r of the time order one 32-byte entry: ts, the payload masked to its length (56 or 112 bits),
//                     and a word of hash | stream << 32 | marker << 56.  marker 0: the record does not take part -- such an
//                     entry matches nothing, so nothing is compacted.  The stream is item_stream[item], the item found by the
//                     binary search over first[] that k_shared_keys uses.
//   k_dedup_find      the hot kernel, one thread per record of the call: is there an earlier-published entry of another
//                     stream with an equal payload and fabs(ts[r] - ts[q]) <= window, in the call (places in front of r) or in
//                     the carry (either side in time)?  A workgroup's 256 consecutive places share one range of the call and
//                     one of the carry -- both found by binary search with the rule's own test, which is monotone along a
//                     sorted list, so the ranges are supersets of what any of its threads accepts -- and stage them through
//                     LDS in tiles of kTile entries: 8 bytes of ts and 8 of hash | stream | marker each, 16 KiB.  Every
//                     thread reads the same element at the same time (an LDS broadcast: no bank conflicts).  Time and the
//                     32-bit hash reject before the 14 payload bytes are read from memory.  The call's range is scanned in
//                     ascending order, so the first match is the earliest-published one, which dup[] names.  The verdict of r
//                     depends on the entries alone, never on another verdict; no atomic is used.  Duplicates lose
//                     ADSB_BURST_DEMOD in the time-ordered copy, so the k_fleet_* kernels skip them.
//   k_dedup_merge     the next carry: a stable merge of the carry and the call's entries into a second buffer (ties: the
//                     carry first), each element's place its own index plus its rank in the other list by binary search on
//                     time_key.  One thread also states hi (the later of the two lists' last ts) and the cut: the entries
//                     with ts < hi - horizon are a prefix, counted in both lists by binary search, so the result is
//                     {offset, count, hi} and nothing is compacted.
//   k_dedup_mark      behind k_shared_scatter: a duplicate's delivered record gets ADSB_BURST_DEMOD back and its row
//                     port = ADSB_DEC_DUPLICATE.
//
// Cost: O(n x entries within window) comparisons of 16 bytes in LDS, + O((n + carry) log) for the ranges and the merge:
// k_dedup_merge reads and rewrites the WHOLE carry every call, one binary search per element.
//
// Records (32 bytes) and rows (72 bytes) are opaque 64-bit words as in adsb_shared_device.h: a record's payload is words 2
// and 3 (bytes 0..7, bytes 8..13 | flags << 48).  Device code only; includes nothing.
#pragma once

namespace adsb_dedup {

constexpr int kThreads = 256;
constexpr int kRecWords = 4, kRowWords = 9, kEntWords = 4;
constexpr int kTile = 1024;                           // entries per LDS tile: 16 bytes each
constexpr int kLdsBytes = kTile * 16 + 16;            // ... and the workgroup's three range bounds
constexpr unsigned long long kFlagDemod = 1ull << 48, kFlagLong = 64ull << 48;      // in record word 3
constexpr unsigned long long kPortDuplicate = 4ull;   // ADSB_DEC_DUPLICATE, byte 0 of row word 0
constexpr int kDupNone = -1, kDupEarlier = -2;

// what k_dedup_merge leaves for the host: the next carry is out[off .. off + cnt)
struct State { int off, cnt; double hi; };

// adsb_shared_device.h's map: ascending keys <=> ascending doubles, -0.0 with +0.0
__device__ __forceinline__ unsigned long long time_key(double ts) {
  unsigned long long b = (unsigned long long)__double_as_longlong(ts);
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ent_ts(const unsigned long long* e, int i) { return __longlong_as_double((long long)e[(long long)i * kEntWords]); }
__device__ __forceinline__ unsigned long long ent_key(const unsigned long long* e, int i) { return time_key(ent_ts(e, i)); }
// THE test of the rule, in double, with exactly this expression
__device__ __forceinline__ bool within(double a, double b, double window) { return __builtin_fabs(a - b) <= window; }
__device__ __forceinline__ unsigned hash32(unsigned long long a, unsigned long long b) {
  unsigned long long k = a ^ (b * 0x9E3779B97F4A7C15ull);
  k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; k ^= k >> 33;
  return (unsigned)k;
}

// first[0 .. n_items], item_stream[n_items]; order[r]: the list position of place r (k_shared_gather)
__global__ void __launch_bounds__(kThreads) k_dedup_entries(const unsigned long long* sorted_recs, const double* sorted_ts, const int* order,
                                                            int n, const int* first, const int* item_stream, int n_items,
                                                            unsigned long long* ent) {
  for (int r = (int)(blockIdx.x * kThreads + threadIdx.x); r < n; r += (int)(gridDim.x * kThreads)) {
    const int t = order[r];
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {                                 // the last item whose first record is not behind t
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const unsigned long long w2 = sorted_recs[(long long)r * kRecWords + 2], w3 = sorted_recs[(long long)r * kRecWords + 3];
    const bool part = (w3 & kFlagDemod) != 0, lng = (w3 & kFlagLong) != 0;
    const unsigned long long a = !part ? 0ull : lng ? w2 : (w2 & 0x00FFFFFFFFFFFFFFull);       // bytes 0..6 of a short reply
    const unsigned long long b = part && lng ? (w3 & 0xFFFFFFFFFFFFull) : 0ull;
    const unsigned long long marker = !part ? 0ull : lng ? 2ull : 1ull;
    unsigned long long* e = ent + (long long)r * kEntWords;
    e[0] = (unsigned long long)__double_as_longlong(sorted_ts[r]);
    e[1] = a;
    e[2] = b;
    e[3] = (unsigned long long)hash32(a, b) | ((unsigned long long)((unsigned)item_stream[lo] & 0xFFFFFFu) << 32) | (marker << 56);
  }
}

// does the staged entry (tq, mq) pass everything but the payload bytes against (ts, m)?
__device__ __forceinline__ bool dedup_near(double ts, unsigned long long m, double tq, unsigned long long mq, double window) {
  if (!within(ts, tq, window)) return false;
  const unsigned long long x = m ^ mq;
  return (x & 0xFF000000FFFFFFFFull) == 0ull && (x & 0x00FFFFFF00000000ull) != 0ull;      // hash and length equal, streams differ
}

// ent[n]: the call's entries in time order; carry[nc]: those of earlier calls.  dup[] is written at LIST positions.
__global__ void __launch_bounds__(kThreads) k_dedup_find(const unsigned long long* ent, int n, const unsigned long long* carry, int nc,
                                                         double window, const int* order, unsigned long long* sorted_recs, int* dup) {
  __shared__ double tile_ts[kTile];
  __shared__ unsigned long long tile_meta[kTile];
  __shared__ int range[4];
  for (int base = (int)blockIdx.x * kThreads; base < n; base += (int)gridDim.x * kThreads) {
    const int r = base + (int)threadIdx.x;
    const int last = (base + kThreads < n ? base + kThreads : n) - 1;      // the workgroup's last place
    if (threadIdx.x == 0) {
      const double t0 = ent_ts(ent, base), t1 = ent_ts(ent, last);
      const unsigned long long k0 = time_key(t0), k1 = time_key(t1);
      int lo = 0, hi = base;                          // the first place of the call within the window of `base`
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (within(t0, ent_ts(ent, mid), window)) hi = mid; else lo = mid + 1; }
      range[0] = lo;
      lo = 0; hi = nc;                                // the first carry entry not in front of t0's window
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ent_key(carry, mid) >= k0 || within(t0, ent_ts(carry, mid), window)) hi = mid; else lo = mid + 1;
      }
      range[1] = lo;
      hi = nc;                                        // ... and the first one behind t1's window
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ent_key(carry, mid) > k1 && !within(t1, ent_ts(carry, mid), window)) hi = mid; else lo = mid + 1;
      }
      range[2] = lo;
    }
    __syncthreads();
    const int q_lo = range[0], c_lo = range[1], c_hi = range[2];
    const bool live = r < n;
    double ts = 0;
    unsigned long long a = 0, b = 0, m = 0;
    if (live) {
      const unsigned long long* e = ent + (long long)r * kEntWords;
      ts = __longlong_as_double((long long)e[0]); a = e[1]; b = e[2]; m = e[3];
    }
    const bool part = live && (m >> 56) != 0;
    bool earlier = false;                             // a match in the carry
    for (int tb = c_lo; tb < c_hi; tb += kTile) {
      const int cnt = c_hi - tb < kTile ? c_hi - tb : kTile;
      for (int j = (int)threadIdx.x; j < cnt; j += kThreads) {
        tile_ts[j] = ent_ts(carry, tb + j);
        tile_meta[j] = carry[(long long)(tb + j) * kEntWords + 3];
      }
      __syncthreads();
      if (part && !earlier)
        for (int j = 0; j < cnt; ++j) {
          if (!dedup_near(ts, m, tile_ts[j], tile_meta[j], window)) continue;
          const unsigned long long* q = carry + (long long)(tb + j) * kEntWords;
          if (q[1] == a && q[2] == b) { earlier = true; break; }
        }
      __syncthreads();
    }
    int best = -1;                                    // the earliest match in the call: a place in front of r
    for (int tb = q_lo; tb < last; tb += kTile) {
      const int cnt = last - tb < kTile ? last - tb : kTile;
      for (int j = (int)threadIdx.x; j < cnt; j += kThreads) {
        tile_ts[j] = ent_ts(ent, tb + j);
        tile_meta[j] = ent[(long long)(tb + j) * kEntWords + 3];
      }
      __syncthreads();
      if (part && !earlier && best < 0) {
        const int stop = r - tb < cnt ? r - tb : cnt;
        for (int j = 0; j < stop; ++j) {
          if (!dedup_near(ts, m, tile_ts[j], tile_meta[j], window)) continue;
          const unsigned long long* q = ent + (long long)(tb + j) * kEntWords;
          if (q[1] == a && q[2] == b) { best = tb + j; break; }
        }
      }
      __syncthreads();
    }
    if (live) {
      const int t = order[r];
      if ((unsigned)t < (unsigned)n) dup[t] = earlier ? kDupEarlier : best >= 0 ? order[best] : kDupNone;
      if (earlier || best >= 0) sorted_recs[(long long)r * kRecWords + 3] &= ~kFlagDemod;
    }
    __syncthreads();                                  // range[] is read by all and rewritten by thread 0 in the next round
  }
}

// entries of e[0 .. n) whose key is below `key` (or_equal: not above it)
__device__ __forceinline__ int dedup_rank(const unsigned long long* e, int n, unsigned long long key, bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const unsigned long long k = ent_key(e, mid);
    if (k < key || (or_equal && k == key)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// out[nc + n]: carry and ent merged, stable, the carry first on equal keys.  *st: the cut at hi - horizon.
__global__ void __launch_bounds__(kThreads) k_dedup_merge(const unsigned long long* carry, int nc, const unsigned long long* ent, int n,
                                                          double horizon, unsigned long long* out, State* st) {
  const int total = nc + n;
  for (int i = (int)(blockIdx.x * kThreads + threadIdx.x); i < total; i += (int)(gridDim.x * kThreads)) {
    const bool old = i < nc;
    const unsigned long long* s = old ? carry + (long long)i * kEntWords : ent + (long long)(i - nc) * kEntWords;
    const unsigned long long key = time_key(__longlong_as_double((long long)s[0]));
    const int pos = old ? i + dedup_rank(ent, n, key, false) : (i - nc) + dedup_rank(carry, nc, key, true);
    unsigned long long* d = out + (long long)pos * kEntWords;
    for (int w = 0; w < kEntWords; ++w) d[w] = s[w];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && total > 0) {
    // the merged list's last entry: the call's, unless the carry's last key is above it
    const bool from_call = n > 0 && (nc == 0 || ent_key(ent, n - 1) >= ent_key(carry, nc - 1));
    const double hi = from_call ? ent_ts(ent, n - 1) : ent_ts(carry, nc - 1);
    const unsigned long long lim = time_key(hi - horizon);       // kept: ts >= hi - horizon
    const int off = dedup_rank(carry, nc, lim, false) + dedup_rank(ent, n, lim, false);
    st->off = off; st->cnt = total - off; st->hi = hi;
  }
}

// dup[n] at list positions; recs / rows: the delivered ones, behind k_shared_scatter
__global__ void __launch_bounds__(kThreads) k_dedup_mark(const int* dup, int n, unsigned long long* recs, unsigned long long* rows) {
  for (int t = (int)(blockIdx.x * kThreads + threadIdx.x); t < n; t += (int)(gridDim.x * kThreads)) {
    if (dup[t] == kDupNone) continue;
    recs[(long long)t * kRecWords + 3] |= kFlagDemod;
    rows[(long long)t * kRowWords] = (rows[(long long)t * kRowWords] & ~0xFFull) | kPortDuplicate;
  }
}

}  // namespace adsb_dedup
