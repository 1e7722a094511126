// softfec_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program for AddressSanitizer and
// UndefinedBehaviorSanitizer on the CPU (tools/softfec_sanitize.sh): the shipped translation unit adsb_softfec.hip -- the host rule
// adsb_mode_s_soft_fec, the real launchers and, on the SIMT emulator, the kernels of adsb_softfec_device.h -- compiled by the host
// compiler against tests/sim/hipstub.  Replies with zero to five wrong bits among their weakest, in all five input formats, at two
// rates, under the default rule, the caps and n_weak = 1, with bursts that leave the buffer at either end, a list shorter than
// its capacity and a mirror shorter than the list: every record, row and slice the kernels write equals the host rule's answer
// for the keys the format's own samples give, and nothing past the delivered records is touched.  Exit status 0: all equal.
#include "../../gr_adsb_amd/csrc/adsb_softfec.hip"

#include <stdio.h>

#include <vector>

namespace {
int failures = 0, repaired = 0;
void expect(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}
unsigned long long lcg = 88172645463325252ull;
unsigned next() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg >> 33); }

int bit_of(const uint8_t* b, int i) { return (b[i >> 3] >> (7 - (i & 7))) & 1; }
void flip(uint8_t* b, int i) { b[i >> 3] ^= (uint8_t)(0x80u >> (i & 7)); }

// a parity-consistent reply of a DF of the parity/interrogator set; 14 bytes (a short reply: random bits behind bit 55)
void make_frame(int df, uint8_t b[14]) {
  static constexpr adsb::CrcTab tab = adsb::make_crc_tab();
  for (int k = 0; k < 14; ++k) b[k] = (uint8_t)next();
  b[0] = (uint8_t)((df << 3) | (b[0] & 7));
  const int L = df == 11 ? 56 : 112;
  for (int i = L - 24; i < L; ++i) if (bit_of(b, i)) flip(b, i);
  unsigned syn = 0;
  for (int i = 0; i < L; ++i) if (bit_of(b, i)) syn ^= tab.r[L - 1 - i];
  for (int i = 0; i < 24; ++i) if ((syn >> (23 - i)) & 1) flip(b, L - 24 + i);
}

template <int MODE>
void keys_of(const void* data, long long n, float scale, int sps, long long p, float key[112]) {
  for (int i = 0; i < 112; ++i) {
    const long long s1 = p + 8ll * sps + (long long)i * sps;
    key[i] = adsb_softfec::soft_key(adsb::xg<MODE>(data, n, s1, scale), adsb::xg<MODE>(data, n, s1 + sps / 2, scale));
  }
}
void keys_by_mode(int mode, const void* data, long long n, float scale, int sps, long long p, float key[112]) {
  switch (mode) {
    case 0: keys_of<0>(data, n, scale, sps, p, key); break;
    case 1: keys_of<1>(data, n, scale, sps, p, key); break;
    case 2: keys_of<2>(data, n, scale, sps, p, key); break;
    case 3: keys_of<3>(data, n, scale, sps, p, key); break;
    default: keys_of<4>(data, n, scale, sps, p, key); break;
  }
}

struct Rec { long long off; float peak, med; uint8_t bits[14]; unsigned short flags; };
static_assert(sizeof(Rec) == 32, "record layout");

void run(int mode, int sps, const adsb_soft_fec_rule& rule, unsigned grid) {
  const long long n = 1 << 12, origin = 5000;
  const int bytes = mode == 0 ? 8 : mode == 1 ? 4 : mode == 2 ? 4 : 2;
  std::vector<unsigned char> data((size_t)n * bytes);
  if (mode <= 1) {
    float* f = (float*)data.data();
    for (size_t k = 0; k < data.size() / 4; ++k) f[k] = (float)(next() & 0xFFFF) / 65536.0f - (mode == 0 ? 0.5f : 0.0f);
  } else {
    for (auto& v : data) v = (unsigned char)next();
  }
  const float scale = mode == 2 ? 1.0f / 32768.0f : mode == 3 ? 1.0f / 128.0f : mode == 4 ? 1.0f / 255.0f : 1.0f;
  const int n_kept = 37, cap = 41, mirror_cap = 19, before = repaired;
  std::vector<Rec> recs(cap), want(cap);
  std::vector<adsb_soft_fix> want_rows(cap);
  const int dfs[5] = {17, 11, 18, 19, 20};
  for (int t = 0; t < cap; ++t) {
    Rec& r = recs[t];
    const long long p = t == 0 ? -40 : t == 1 ? n - 60 : (long long)(next() % (unsigned)(n - 120 * sps));
    r.off = origin + p; r.peak = 1.0f; r.med = 0.1f;
    const int df = dfs[t % 5];
    make_frame(df == 20 ? 17 : df, r.bits);
    float key[112];
    keys_by_mode(mode, data.data(), n, scale, sps, p, key);
    // wrong bits: the t % 6 weakest candidates by the host's own ordering of those keys
    int order[112], no = 0;
    for (int i = 5; i < (df == 11 ? 56 : 112); ++i) order[no++] = i;
    for (int i = 1; i < no; ++i)
      for (int k = i; k > 0 && key[order[k - 1]] < key[order[k]]; --k) { const int q = order[k]; order[k] = order[k - 1]; order[k - 1] = q; }
    for (int w = 0; w < t % 6; ++w) flip(r.bits, order[w]);
    if (df == 20) r.bits[0] = (uint8_t)((20 << 3) | (r.bits[0] & 7));
    // the raw record's pre-filter bits: those of its own bits (a NULL key: the rule does not run)
    const uint32_t fl = adsb_mode_s_soft_fec(r.bits, nullptr, nullptr, nullptr, nullptr);
    r.flags = (unsigned short)(ADSB_BURST_DEMOD | ADSB_BURST_KEPT | fl);
    if (t % 11 == 7) r.flags &= (unsigned short)~ADSB_BURST_DEMOD;
    if (t % 13 == 5) r.flags |= ADSB_BURST_FEC_DF;
    want[t] = r;
    memset(&want_rows[t], 0, sizeof(adsb_soft_fix));
    const bool pi = df != 20;
    if (t < n_kept && (r.flags & ADSB_BURST_DEMOD) && !(r.flags & (ADSB_BURST_PARITY_OK | ADSB_BURST_FEC_DF)) && pi) {
      const uint32_t f2 = adsb_mode_s_soft_fec(r.bits, key, &rule, want[t].bits, &want_rows[t]);
      if (f2 & ADSB_BURST_FEC_FIXED) {
        const unsigned keep = r.flags & ~(ADSB_BURST_PARITY_OK | ADSB_BURST_LONG | ADSB_BURST_KNOWN_DF | (31u << ADSB_BURST_DF_SHIFT));
        want[t].flags = (unsigned short)(keep | f2);
        ++repaired;
      }
    }
  }
  // (one to three wrong bits among the eight weakest: the default rule and the caps repair some in every run)
  if (rule.n_weak >= 8 && rule.min_key == 0.0f) expect(repaired > before, "the host rule repaired a reply");
  // the record kernel through its launcher
  std::vector<Rec> list = recs, mirror(recs.begin(), recs.begin() + mirror_cap);
  std::vector<adsb_soft_fix> rows(cap);
  memset(rows.data(), 0xEE, rows.size() * sizeof(adsb_soft_fix));
  const int kept = n_kept;
  expect(adsb_softfec_host::launch_records(nullptr, grid, mode, data.data(), n, origin, scale, sps, &rule, list.data(), &kept, cap, mirror.data(),
                                           mirror_cap, rows.data()) == 0, "launch_records");
  expect(memcmp(list.data(), want.data(), (size_t)n_kept * sizeof(Rec)) == 0, "records equal the host rule");
  expect(memcmp(list.data() + n_kept, recs.data() + n_kept, (size_t)(cap - n_kept) * sizeof(Rec)) == 0, "records past n_kept untouched");
  expect(memcmp(mirror.data(), want.data(), (size_t)mirror_cap * sizeof(Rec)) == 0, "mirror equals the host rule");
  expect(memcmp(rows.data(), want_rows.data(), (size_t)n_kept * sizeof(adsb_soft_fix)) == 0, "rows equal the host rule");
  for (int t = n_kept; t < cap; ++t) expect(rows[t].nflip == 0xEE && rows[t].pad == 0xEE, "rows past n_kept untouched");
  // the slices kernel on the same replies (float input only)
  if (mode != 1) return;
  std::vector<unsigned char> bits14((size_t)n_kept * 14), ok(n_kept);
  std::vector<long long> tags(n_kept);
  std::vector<adsb_soft_fix> srows(n_kept);
  for (int t = 0; t < n_kept; ++t) {
    memcpy(&bits14[(size_t)t * 14], recs[t].bits, 14);
    ok[t] = (unsigned char)((recs[t].flags & 0xE1u) | ((recs[t].flags & (ADSB_BURST_FEC_FIXED | ADSB_BURST_FEC_DF)) >> 13));
    tags[t] = recs[t].off - origin;
  }
  expect(adsb_softfec_host::launch_slices(nullptr, grid, data.data(), n, tags.data(), sps, &rule, bits14.data(), ok.data(), n_kept, srows.data()) == 0,
         "launch_slices");
  for (int t = 0; t < n_kept; ++t) {
    expect(memcmp(&bits14[(size_t)t * 14], want[t].bits, 14) == 0, "slice bits equal the host rule");
    expect(ok[t] == (unsigned char)((want[t].flags & 0xE1u) | ((want[t].flags & (ADSB_BURST_FEC_FIXED | ADSB_BURST_FEC_DF)) >> 13)), "ok[] equals the host rule");
  }
  expect(memcmp(srows.data(), want_rows.data(), (size_t)n_kept * sizeof(adsb_soft_fix)) == 0, "slice rows equal the host rule");
}
}  // namespace

int main() {
  const adsb_soft_fec_rule rules[4] = {{8, 3, 0.0f, 0u}, {16, 5, 0.0f, 0u}, {1, 1, 0.0f, 0u}, {8, 3, 0.4f, 0u}};
  for (int mode = 0; mode < 5; ++mode)
    for (int sps : {2, 10})
      for (const adsb_soft_fec_rule& r : rules)
        for (unsigned grid : {1u, 3u}) run(mode, sps, r, grid);
  // the launchers' argument edges: nothing to do
  expect(adsb_softfec_host::launch_records(nullptr, 1, 1, nullptr, 0, 0, 1.0f, 2, &rules[0], nullptr, nullptr, 0, nullptr, 0, nullptr) == 0, "empty list");
  expect(adsb_softfec_host::launch_slices(nullptr, 1, nullptr, 0, nullptr, 2, &rules[0], nullptr, nullptr, 0, nullptr) == 0, "no tags");
  expect(adsb_softfec_host::launch_records(nullptr, 1, 9, nullptr, 0, 0, 1.0f, 2, &rules[0], nullptr, nullptr, 1, nullptr, 0, nullptr) != 0, "unknown format");
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("softfec sanitize: ok\n");
  return 0;
}
