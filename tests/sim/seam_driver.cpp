// seam_driver.cpp -- TEST INFRASTRUCTURE ONLY.  The library's seam consumer (gr_adsb_amd/csrc/adsb_seam.h: the code both
// sharded drivers run between two shards) over shards given as record lists, with a fake re-run in place of a device pass.
// Every shard comes as THREE lists: as a pass with the first head delivered it, as one with a second head did, and ungated.
// The fake re-run hands out the second list when the consumer asks for the largest head and the third when it asks for
// head 0 -- a short list standing in for "4096" is what lets a small shard reach the ungated step.
#include <cstdint>
#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_seam.h"

// recs: all lists one after the other, list v of shard g = recs[start[3g+v] .. start[3g+v+1]) (start: 3*n_shards+1 entries).
// fail_shard >= 0: the re-run of that shard asked for head `fail_head` returns fail_code (and the run ends there).
// Out: the consumer's records in out[0..min(total, cap)), its total / eob / fallback count, what the final step wrote and
// returned, and per shard the outcome: 0 synchronised at once, 1 with the second head, 2 ungated (-1: not reached).
// Returns 0, or what take() returned.
extern "C" int seam_run(const adsb_burst* recs, const int64_t* start, int n_shards, int sps, int64_t abs_offset, adsb_burst* out,
                        int32_t cap, int fail_shard, int fail_head, int fail_code, int64_t* total, int64_t* eob, int* fallbacks,
                        int32_t* n_out, int* finish_rc, int* outcome) {
  adsb::SeamConsumer seam{sps, out, cap, abs_offset};
  for (int g = 0; g < n_shards; ++g) outcome[g] = -1;
  int rc = 0;
  for (int g = 0; g < n_shards && !rc; ++g) {
    std::vector<adsb_burst> list[3];
    for (int v = 0; v < 3; ++v) list[v].assign(recs + start[3 * g + v], recs + start[3 * g + v + 1]);
    int asked = 0;
    auto rerun = [&](int head_cands, adsb_burst** rr, int32_t* nn) -> int {
      if (head_cands != adsb::kHeadMax && head_cands != 0) return -1000;      // the consumer asks for these two only
      if (g == fail_shard && head_cands == fail_head) return fail_code;
      asked = head_cands == adsb::kHeadMax ? 1 : 2;
      *rr = list[asked].data(); *nn = (int32_t)list[asked].size();
      return 0;
    };
    int32_t kept = 0;
    rc = seam.take(list[0].data(), (int32_t)list[0].size(), rerun, &kept);
    if (!rc) outcome[g] = asked;
  }
  *total = seam.total; *eob = seam.eob; *fallbacks = seam.fallbacks;
  *n_out = -1;
  *finish_rc = rc ? 0 : seam.finish(n_out);
  return rc;
}

extern "C" int seam_head_first() { return adsb::kHeadFirst; }
extern "C" int seam_head_max() { return adsb::kHeadMax; }
