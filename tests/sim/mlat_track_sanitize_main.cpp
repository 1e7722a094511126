// mlat_track_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program around mlat_track_driver.cpp for AddressSanitizer
// and UndefinedBehaviorSanitizer on the CPU (tools/mlat_track_sanitize.sh): adsb_mlat_track.h's sizing rule over the sizes at
// which a part's length crosses a 256-byte boundary, a chunk or a sort tile, and tests/test_mlat_track.py's kinds of call through
// the real launchers and the emulated kernels -- no fix, ineligible and unusable fixes, 5000 fixes of 700 addresses into an empty
// store and again into the store they left (every fix stale, the store byte-identical), a run of 300, new addresses below,
// between and above old ones, the readout with its filters, the count query and -ENOSPC, the expiry, the argument table.
// Exit status 0: every call returned what it should.
#include "mlat_track_driver.cpp"

#include <cmath>
#include <set>

namespace {
namespace tk = adsb_mlat_track;

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}

unsigned long long lcg = 88172645463325252ull;
unsigned next() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg >> 33); }

struct Fixes {
  std::vector<tk::Fix> f;
  std::vector<tk::Aux> a;
  void add(int icao, double ts, double x, double y, double z, int status = 0, double rms = 10.0, double up = 100.0) {
    tk::Fix q{};
    q.ts = ts; q.x = x; q.y = y; q.z = z; q.rms_m = rms; q.icao = icao; q.n_rx = 4; q.status = status;
    tk::Aux u{};
    u.up_m = up; u.alt_ft = -1;
    f.push_back(q); a.push_back(u);
  }
};

struct Store {
  std::vector<tk::Track> rows;
  long long stats[8] = {0};
};

const tk::Rule kRule = {0.3, 0.05, 2000.0, 350.0, 30.0, 500.0, 0.0, 3, 0};

int update(const Fixes& in, const Store& before, Store& after, const tk::Rule& rule = kRule, bool with_aux = true) {
  const int ng = (int)in.f.size(), nt = (int)before.rows.size();
  std::vector<tk::Track> out((size_t)nt + (size_t)ng + 1);
  int n = -1;
  const int rc = sim_track_update(in.f.data(), with_aux ? in.a.data() : nullptr, ng, &rule, before.rows.data(), nt, out.data(), &n, after.stats);
  if (rc == 0) after.rows.assign(out.begin(), out.begin() + n);
  return rc;
}

bool ascending(const Store& s) {
  for (size_t k = 1; k < s.rows.size(); ++k) if (s.rows[k - 1].icao >= s.rows[k].icao) return false;
  return true;
}
bool same(const Store& a, const Store& b) {
  return a.rows.size() == b.rows.size() && (a.rows.empty() || memcmp(a.rows.data(), b.rows.data(), a.rows.size() * sizeof(tk::Track)) == 0);
}
}  // namespace

int main() {
  static_assert(sizeof(tk::Track) == 96 && sizeof(tk::Rule) == 64 && sizeof(tk::Fix) == 88 && sizeof(tk::Aux) == 32, "the ABI's sizes");
  for (long long n : {0ll, 1ll, 63ll, 64ll, 65ll, 255ll, 256ll, 257ll, 4095ll, 4096ll, 4097ll, 100000ll}) {
    unsigned long long offs[14];
    const unsigned long long total = sim_track_layout(n, offs);
    bool ok = offs[0] == 0 && total % 256 == 0;
    for (int k = 1; k < 14; ++k) ok = ok && offs[k] % 256 == 0 && offs[k] >= offs[k - 1];
    ok = ok && offs[2] - offs[1] == 256 && offs[3] - offs[2] == (unsigned long long)((n * 4 + 255) / 256 * 256) &&
         total - offs[13] == (unsigned long long)((n + 4095) / 4096 * 1024);
    expect(ok, "the sizing rule");
  }
  expect(sim_track_cover(0, 256) == 1 && sim_track_cover(257, 256) == 2 && sim_track_cover(1ll << 40, 256) == 2048, "cover()");

  Store empty, s1, s2, s3;
  {
    Fixes none;
    expect(update(none, empty, s1) == 0 && s1.rows.empty() && s1.stats[0] == 0, "no fix");
    Fixes bad;
    bad.add(-1, 1.0, 1, 2, 3);
    bad.add(7, 2.0, NAN, 2, 3);
    bad.add(7, 3.0, 1, 2, 3, 1);
    bad.add(8, 4.0, 1, 2, 3, 0, 600.0);
    bad.add(9, 5.0, 1, 2, 3, 0, 10.0, -1.0);
    expect(update(bad, empty, s1) == 0 && s1.rows.empty() && s1.stats[1] == 4 && s1.stats[2] == 4 && s1.stats[7] == 0, "ineligible and unusable fixes");
    expect(update(bad, empty, s1, kRule, false) == 0 && s1.rows.size() == 1 && s1.rows[0].icao == 9, "without aux rows up_m is 0");
  }
  {
    Fixes many;
    std::vector<int> addr;
    std::set<int> seen;
    while (addr.size() < 700) { const int a = (int)(next() & 0xFFFFFFu); if (seen.insert(a).second) addr.push_back(a); }
    seen.clear();
    for (int k = 0; k < 5000; ++k) {
      const int who = (int)(next() % 700u);
      const bool far = false, unusable = next() % 30u == 0;      // (a rejected fix is not remembered: a second call would gate it again)
      many.add(next() % 20u == 0 ? -1 : addr[(size_t)who], k * 0.01, 4e6 + who * 1e3 + (far ? 5e4 : 0.0) + (next() % 200u), who * 10.0, 5e6 + (next() % 100u),
               unusable ? 2 : 0);
      if (many.f.back().icao >= 0 && !unusable) seen.insert(many.f.back().icao);
    }
    expect(update(many, empty, s1) == 0 && ascending(s1) && s1.rows.size() == seen.size() && s1.stats[7] == (long long)seen.size(), "5000 fixes of 700 addresses");
    expect(s1.stats[0] == 5000 && s1.stats[6] >= (long long)seen.size() && s1.stats[5] > 0 && s1.stats[3] == 0, "... their totals");
    expect(update(many, s1, s2) == 0 && same(s1, s2) && s2.stats[3] == s2.stats[1] - s2.stats[2] && s2.stats[5] == 0 && s2.stats[6] == 0,
           "a second identical call: every usable fix is stale and the store is the same bytes");
    Fixes more;                                       // new addresses below, between and above, a run of 300, and old addresses again
    for (int k = 0; k < 300; ++k) more.add(0x123456, 100.0 + k, 4e6 + 200.0 * k, 1e5, 5e6);
    more.add(0, 100.0, 1, 2, 3);
    more.add(0xFFFFFF, 100.0, 1, 2, 3);
    more.add(s1.rows[3].icao, s1.rows[3].last_ts + 1.0, s1.rows[3].x + 5e4, s1.rows[3].y, s1.rows[3].z);      // an outlier: rejected
    for (size_t k = 0; k < s1.rows.size(); k += 7) more.add(s1.rows[k].icao, 200.0, s1.rows[k].x, s1.rows[k].y, s1.rows[k].z);
    const size_t fresh = (seen.count(0x123456) ? 0 : 1) + (seen.count(0) ? 0 : 1) + (seen.count(0xFFFFFF) ? 0 : 1);
    expect(update(more, s1, s3) == 0 && ascending(s3) && s3.rows.size() == s1.rows.size() + fresh && s3.rows.front().icao == 0 && s3.rows.back().icao == 0xFFFFFF &&
               s3.stats[4] == 1,
           "the merge");
    bool run_ok = false;
    for (const tk::Track& t : s3.rows) if (t.icao == 0x123456) run_ok = t.n_fixes == 300 && std::fabs(t.vx - 200.0) < 1.0;
    expect(run_ok, "a run of 300 fixes at 200 m/s");
  }
  {
    const int nt = (int)s3.rows.size();
    std::vector<tk::Track> out((size_t)nt + 1);
    int n = -1;
    expect(sim_track_read(s3.rows.data(), nt, 1, -INFINITY, out.data(), nt, &n) == 0 && n == nt && memcmp(out.data(), s3.rows.data(), (size_t)nt * 96) == 0,
           "the readout of everything");
    int n3 = -1;
    expect(sim_track_read(s3.rows.data(), nt, 3, -INFINITY, nullptr, 0, &n3) == (n3 ? -28 : 0) && n3 >= 1 && n3 < nt, "the count query");
    expect(sim_track_read(s3.rows.data(), nt, 3, -INFINITY, out.data(), n3 - 1, &n) == -28 && n == n3, "-ENOSPC");
    expect(sim_track_read(s3.rows.data(), nt, 3, 150.0, out.data(), nt, &n) == 0 && n >= 1 && out[0].n_fixes >= 3 && out[0].last_ts >= 150.0, "the filters");
    expect(sim_track_read(s3.rows.data(), nt, 1, NAN, out.data(), nt, &n) == -22 && sim_track_read(s3.rows.data(), nt, 1, 0.0, nullptr, 4, &n) == -22, "the readout's arguments");
    int kept = -1;
    expect(sim_track_expire(s3.rows.data(), nt, 200.0, out.data(), &kept) == 0 && kept >= 1 && kept < nt, "the expiry");
    for (int k = 0; k < kept; ++k) expect(out[(size_t)k].last_ts >= 200.0, "... keeps last_ts >= cutoff");
    expect(sim_track_expire(s3.rows.data(), nt, INFINITY, out.data(), &kept) == 0 && kept == 0, "... of everything");
    expect(sim_track_expire(s3.rows.data(), nt, -INFINITY, out.data(), &kept) == 0 && kept == nt, "... of nothing");
  }
  {
    Fixes one;
    one.add(5, 1.0, 1, 2, 3);
    Store out;
    tk::Rule r = kRule;
    r.alpha = 0.0;
    expect(update(one, empty, out, r) == -22, "alpha 0");
    r = kRule; r.beta = NAN;
    expect(update(one, empty, out, r) == -22, "beta NaN");
    r = kRule; r.gate_m = -1.0;
    expect(update(one, empty, out, r) == -22, "gate_m < 0");
    r = kRule; r.restart_after = 0;
    expect(update(one, empty, out, r) == -22, "restart_after 0");
    r = kRule; r.reserved = 1;
    expect(update(one, empty, out, r) == -22, "reserved");
    int n = -1;
    long long st[8];
    tk::Track row;
    expect(sim_track_update(one.f.data(), one.a.data(), 1, nullptr, nullptr, 0, &row, &n, st) == -22, "no rule");
    expect(update(one, empty, out) == 0 && out.rows.size() == 1, "one fix");
  }
  if (failures) return 1;
  printf("mlat_track_sanitize: ok\n");
  return 0;
}
