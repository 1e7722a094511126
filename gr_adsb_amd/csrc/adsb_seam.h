// adsb_seam.h -- what crosses the seam between two overlapped time shards, shared by libadsb_hip.so (both sharded
// drivers, adsb_shard_fixup, adsb_stitch) and the test driver tests/sim/seam_driver.cpp.  Pure C++, no HIP: the host gates
// over delivered records and the ONE consumer that takes a sharded call's shards in stream order.
// Citations: framer.py of the reference.
#pragma once

#include <cerrno>
#include <cstring>

#include "adsb_plan.h"

namespace adsb {

// head_cands of a sharded call's passes: every shard first, and the largest a shard is run again with
constexpr int kHeadFirst = 64, kHeadMax = 4096;
constexpr long long kSeamNoEob = -(1ll << 60);          // the state in front of the first shard: gates nothing

inline int shard_fixup(adsb_burst* recs, int32_t n, int sps, long long eob_in, int32_t* n_kept, bool* open_end = nullptr) {
  // recs: output of adsb_shard_device(head_cands > 0): every centre of the shard's head (ADSB_BURST_HEAD,
  // complete, gated or not) followed by the centres a fresh-state gate kept.  Re-gate the head with the
  // true incoming eob (framer.py:121-123,165) until the first centre that starts an independent chain
  // -- beyond the reach (offset + gate window) of every head centre before it (trivially true for the first one)
  // and beyond eob_in: it is accepted whatever came before, so from there on the fresh-state decisions are exact.
  // A shard that lies entirely in its head region is re-gated completely and never fails; whether its END-OF-BURST
  // state equals the fresh-state one is a separate question the caller answers with the same criterion
  // (gr_adsb_amd/_native.py shard_head_sync; sharding.finish_shard falls back to adsb_stitch when it does not).
  // The window of a record: gate_window (adsb_plan.h).
  int i = 0, w = 0;
  long long eob = eob_in, reach = -(1ll << 61);
  bool synced = false;
  for (; i < n && (recs[i].flags & ADSB_BURST_HEAD); ++i) {
    const long long p = recs[i].offset;
    const long long gate = gate_window(recs[i].flags, sps);
    if (p > reach && p > eob_in) { synced = true; break; }   // also i == 0: the first centre lies beyond eob_in
    if (p + gate > reach) reach = p + gate;
    if (p > eob) {
      eob = p + gate;
      adsb_burst b = recs[i];
      b.flags = (uint16_t)((b.flags | ADSB_BURST_KEPT) & ~ADSB_BURST_HEAD);
      recs[w++] = b;
    }
  }
  if (!synced && i < n) return -EAGAIN;   // the head region ended inside a chain: ask for a larger head
  // *open_end: the LIST ended inside a chain that began at or before eob_in.  Exact for a shard that lies entirely in its
  // head region; behind a FULL head the pass may have dropped centres on account of a head centre the true state does not
  // keep, and the list cannot tell the two apart (the seam consumer asks again; the exports answer as they always have)
  if (open_end) *open_end = !synced && n > 0;
  for (; i < n; ++i) {
    if (!(recs[i].flags & ADSB_BURST_KEPT)) continue;
    adsb_burst b = recs[i];
    b.flags = (uint16_t)(b.flags & ~ADSB_BURST_HEAD);
    recs[w++] = b;
  }
  *n_kept = w;
  return 0;
}

inline int stitch(adsb_burst* cands, int32_t n, int sps, int32_t* n_kept) {
  long long eob = -(1ll << 61);
  int w = 0;
  for (int i = 0; i < n; ++i) {
    if (i > 0 && cands[i].offset <= cands[i - 1].offset) return -EINVAL;  // must be in stream order
    if (cands[i].offset > eob) {                                           // framer.py:121
      eob = cands[i].offset + gate_window(cands[i].flags, sps);
      adsb_burst b = cands[i];
      b.flags |= ADSB_BURST_KEPT;
      cands[w++] = b;
    }
  }
  if (n_kept) *n_kept = w;
  return 0;
}

// the plain greedy gate (framer.py:121-123,165) over a shard's UNGATED centres with the incoming end-of-burst state: the
// fallback for a shard whose head region ends inside an unbroken chain of overlapping bursts
inline int32_t gate_from(adsb_burst* recs, int32_t n, int sps, long long* eob_io) {
  long long eob = *eob_io;
  int32_t w = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (recs[i].offset > eob) {
      eob = recs[i].offset + gate_window(recs[i].flags, sps);
      adsb_burst b = recs[i];
      b.flags = (uint16_t)((b.flags | ADSB_BURST_KEPT) & ~ADSB_BURST_HEAD);
      recs[w++] = b;
    }
  }
  *eob_io = eob;
  return w;
}

// The seam consumer of a sharded call: takes the shards' records in STREAM order (each as a pass with head kHeadFirst
// delivered them), re-gates every head with the end-of-burst state carried over the seam -- the only thing that crosses
// it is this one int64 -- and appends what is kept to `out`.  How a shard is run again and how an error is reported is
// the caller's: the consumer knows no context, slot or thread.
struct SeamConsumer {
  int sps;
  adsb_burst* out;
  int32_t cap;
  int64_t abs_offset;
  long long eob = kSeamNoEob;
  int64_t total = 0;          // records kept so far, whether `out` had room for them or not
  int fallbacks = 0;          // shards whose first head ended inside a chain

  // One shard's records, fixed up in place.  A head that ends inside a chain (-EAGAIN) has its shard run again:
  // rerun(head_cands, &recs, &n) -> 0 or an error, first with the largest head, then with head 0 = ungated, for the plain
  // greedy gate (exact in every case).  An error of rerun is returned as it came; the shard then appends nothing and the
  // carried state stands as it was.  *kept: how many of recs[] were kept.
  template <class Rerun>
  int take(adsb_burst* recs, int32_t n, Rerun&& rerun, int32_t* kept_out) {
    int32_t kept = 0;
    // (a list that ends inside the chain it began in counts as too short a head: the consumer does not know whether the
    // head was full, and the ungated step is exact whatever it was)
    auto fixup = [&]() { bool open = false; const int e = shard_fixup(recs, n, sps, eob, &kept, &open); return open ? -EAGAIN : e; };
    int r = fixup();
    if (r == -EAGAIN) {
      if ((r = rerun(kHeadMax, &recs, &n))) return r;
      if ((r = fixup()) == -EAGAIN) {
        if ((r = rerun(0, &recs, &n))) return r;
        long long e = eob;
        kept = gate_from(recs, n, sps, &e);
      }
      if (r) return r;
      ++fallbacks;
    } else if (r) return r;
    if (kept > 0) {
      const adsb_burst& last = recs[kept - 1];
      eob = last.offset + gate_window(last.flags, sps);
      if (total + kept <= cap) {
        memcpy(out + total, recs, (size_t)kept * sizeof(adsb_burst));
        if (abs_offset) for (int32_t i = 0; i < kept; ++i) out[total + i].offset += abs_offset;
      }
    }
    total += kept;
    *kept_out = kept;
    return 0;
  }

  // after the last shard: the number of records the call kept (as far as an int32 states it), -ENOSPC when `out` was too
  // small for them
  int finish(int32_t* n_out) const {
    *n_out = (int32_t)(total > 0x7FFFFFFF ? 0x7FFFFFFF : total);
    return total > cap ? -ENOSPC : 0;
  }
};

}  // namespace adsb
