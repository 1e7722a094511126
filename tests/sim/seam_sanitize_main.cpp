// seam_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program around seam_driver.cpp for AddressSanitizer and
// UndefinedBehaviorSanitizer on the CPU (tools/seam_sanitize.sh): the library's seam consumer (gr_adsb_amd/csrc/adsb_seam.h)
// over a few hundred generated worlds -- matched centres in chains and gaps, cut into shards anywhere, every shard as a pass
// with a head of 1..3 centres, one with a head of 4 or 8 and ungated -- with an output array from too small to large enough,
// against a plain sequential gate written here.  Exit status 0: every world came out as that gate has it.
#include "seam_driver.cpp"

#include <cstdio>

namespace {
int failures = 0;
void expect(bool ok, const char* what, int world) {
  if (!ok) { fprintf(stderr, "FAILED (world %d): %s\n", world, what); ++failures; }
}

unsigned long long lcg_state = 0x9E3779B97F4A7C15ull;
unsigned lcg(unsigned n) {                      // 0 .. n-1
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((lcg_state >> 33) % n);
}

long long window(const adsb_burst& b, int sps) { return ((b.flags & ADSB_BURST_LONG_HINT) ? 119 : 63) * (long long)sps; }

// what a shard pass delivers, by its definition: the gate from fresh state (KEPT) and the first head_n centres whether kept
// or not (HEAD); head_n < 0: every centre, no flag
void deliver(const std::vector<adsb_burst>& centres, int sps, int head_n, std::vector<adsb_burst>& to) {
  long long eob = -(1ll << 61);
  for (size_t i = 0; i < centres.size(); ++i) {
    adsb_burst b = centres[i];
    if (head_n >= 0) {
      const bool kept = b.offset > eob, head = (int)i < head_n;
      if (kept) eob = b.offset + window(b, sps);
      if (!kept && !head) continue;
      b.flags = (uint16_t)(b.flags | (kept ? ADSB_BURST_KEPT : 0) | (head ? ADSB_BURST_HEAD : 0));
    }
    to.push_back(b);
  }
}
}  // namespace

int main() {
  const int kSps[4] = {2, 4, 8, 20};
  int outcomes[3] = {0, 0, 0};
  for (int world = 0; world < 400; ++world) {
    const int sps = kSps[lcg(4)], n = (int)lcg(61), n_cuts = (int)lcg(9);
    const bool hints = lcg(2) != 0;
    std::vector<adsb_burst> all((size_t)n);
    long long at = 1000;
    for (int i = 0; i < n; ++i) {
      const unsigned kind = lcg(4);
      at += kind == 0 ? 1 + lcg(3) : kind == 1 ? 63 * sps - 2 + lcg(5) : kind == 2 ? 119 * sps - 2 + lcg(5) : 1 + lcg(3 * 63 * sps);
      all[(size_t)i] = adsb_burst();
      all[(size_t)i].offset = at;
      all[(size_t)i].flags = (uint16_t)(hints && lcg(2) ? ADSB_BURST_LONG_HINT : 0);
      all[(size_t)i].bits[0] = (uint8_t)i;                             // (a record is more than its offset)
    }
    // shard g owns the centres [first[g], first[g + 1])
    std::vector<int> first((size_t)n_cuts + 2, 0);
    for (int k = 1; k <= n_cuts; ++k) first[(size_t)k] = (int)lcg((unsigned)n + 1);
    first[(size_t)n_cuts + 1] = n;
    for (size_t a = 1; a < first.size(); ++a)
      for (size_t b = a + 1; b < first.size(); ++b)
        if (first[b] < first[a]) std::swap(first[a], first[b]);
    const int n_shards = n_cuts + 1, h1 = 1 + (int)lcg(3), h2 = lcg(2) ? 4 : 8;
    std::vector<adsb_burst> recs;
    std::vector<int64_t> start(1, 0);
    for (int g = 0; g < n_shards; ++g) {
      const std::vector<adsb_burst> mine(all.begin() + first[(size_t)g], all.begin() + first[(size_t)g + 1]);
      for (int head : {h1, h2, -1}) { deliver(mine, sps, head, recs); start.push_back((int64_t)recs.size()); }
    }
    // the plain sequential gate over all centres
    std::vector<adsb_burst> want;
    long long eob_want = -(1ll << 60);
    for (const adsb_burst& c : all)
      if (c.offset > eob_want) { want.push_back(c); want.back().flags |= ADSB_BURST_KEPT; eob_want = c.offset + window(c, sps); }
    const int64_t abs_offset = lcg(2) ? 0 : 1000003;
    for (int32_t cap : {(int32_t)0, (int32_t)(want.size() / 2), (int32_t)want.size(), (int32_t)want.size() + 3}) {
      std::vector<adsb_burst> out((size_t)cap);                       // exactly cap records: the sanitizer watches its end
      std::vector<int> outcome((size_t)n_shards);
      int64_t total = 0, eob = 0;
      int fb = 0, frc = 0;
      int32_t n_out = 0;
      const int rc = seam_run(recs.data(), start.data(), n_shards, sps, abs_offset, out.data(), cap, -1, 0, 0, &total, &eob, &fb, &n_out, &frc,
                              outcome.data());
      expect(rc == 0 && total == (int64_t)want.size() && n_out == (int32_t)want.size() && eob == eob_want, "total and carried state", world);
      expect(frc == ((int64_t)want.size() > cap ? -ENOSPC : 0), "-ENOSPC exactly when the array is too small", world);
      int fb_want = 0;
      for (int o : outcome) { fb_want += o > 0; if (o >= 0 && o < 3) ++outcomes[o]; else expect(false, "outcome", world); }
      expect(fb == fb_want, "fallback count", world);
      if (frc == 0)
        for (size_t i = 0; i < want.size(); ++i) {
          adsb_burst w = want[i];
          w.offset += abs_offset;
          expect(memcmp(&w, &out[i], sizeof(w)) == 0, "records", world);
        }
    }
  }
  expect(outcomes[0] > 0 && outcomes[1] > 0 && outcomes[2] > 0, "every outcome occurred", -1);
  printf(failures ? "seam_sanitize: %d failures\n" : "seam_sanitize: ok (%d at once, %d second head, %d ungated)\n",
         failures ? failures : outcomes[0], outcomes[1], outcomes[2]);
  return failures != 0;
}
