// mlat_rule_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program around mlat_rule_driver.cpp for AddressSanitizer
// and UndefinedBehaviorSanitizer on the CPU (tools/mlat_rule_sanitize.sh): adsb_mlat_rule.h's sizing rule over the sizes at which
// a part's length crosses a 256-byte boundary or nc / 3 steps, and tests/test_mlat_rule.py's kinds of call through the emulated
// kernels -- six receivers with the restart, a three-hearing group with an altitude beside one without and a four-hearing
// group, 65 hearings of one reply, all receivers at one point, -ENOSPC, the argument table, and _GN.  Exit status 0: every call
// returned what it should.
#include "mlat_rule_driver.cpp"

#include <cmath>

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}

struct World {
  std::vector<double> ts, rx;
  std::vector<unsigned char> bits;
  std::vector<int> marker, stream;
  // a long reply of DF 17: type code tc, alt_ft in bits 40..51 with Q = 1
  void add(double t, unsigned id, int s, int tc, int alt_ft) {
    ts.push_back(t); marker.push_back(2); stream.push_back(s);
    const unsigned n = (unsigned)(alt_ft + 1000) / 25u, v = ((n >> 4) << 5) | 0x10u | (n & 0xFu);
    unsigned char b[14] = {0x8D, (unsigned char)(id >> 16), (unsigned char)(id >> 8), (unsigned char)id, (unsigned char)(tc << 3),
                           (unsigned char)(v >> 4), (unsigned char)((v & 0xFu) << 4), 4, 5, 6, 7, 8, 9, 10};
    bits.insert(bits.end(), b, b + 14);
  }
  // the carry is time-sorted: order the entries from `from` on among themselves
  void sort_from(size_t from) {
    for (size_t i = from; i < ts.size(); ++i)
      for (size_t j = i + 1; j < ts.size(); ++j)
        if (ts[j] < ts[i]) {
          std::swap(ts[i], ts[j]); std::swap(stream[i], stream[j]);
          for (int k = 0; k < 14; ++k) std::swap(bits[i * 14 + k], bits[j * 14 + k]);
        }
  }
};

// n receivers on a 100 km circle around a point of the ellipsoid's neighbourhood, alternating heights; an aircraft above it
void place(World& w, int n, double p[3]) {
  for (int s = 0; s < n; ++s) {
    const double a = 6.283185307179586 * s / n;
    w.rx.push_back(4.0e6 + 1.0e5 * std::cos(a) - 800.0 * (s % 3));
    w.rx.push_back(1.0e5 * std::sin(a));
    w.rx.push_back(5.0e6 + 1200.0 * (s % 2));
  }
  p[0] = 4.0e6 + 7000.0; p[1] = 12000.0; p[2] = 5.0e6 + 9000.0;
}
double arrival(const World& w, int s, const double p[3], double t) {
  const double dx = p[0] - w.rx[3 * s], dy = p[1] - w.rx[3 * s + 1], dz = p[2] - w.rx[3 * s + 2];
  return t + std::sqrt(dx * dx + dy * dy + dz * dz) / ml::kC;
}

struct Out {
  std::vector<ml::Fix> fixes;
  std::vector<ml::Aux> aux;
  int nf = 0, nm = 0;
};
int run(World& w, int n_streams, int solver, int flags, int min_rx, double weight, int grid, Out& o, int cap = -1, int member_cap = -1) {
  const int nc = (int)w.ts.size();
  o.fixes.assign((size_t)nc / 3 + 1, ml::Fix());
  o.aux.assign((size_t)nc / 3 + 1, ml::Aux());
  std::vector<int> ms((size_t)nc + 1), heads((size_t)nc + 1);
  std::vector<double> mt((size_t)nc + 1);
  int nh = 0;
  return sim_mlat_rule(w.ts.data(), w.bits.data(), w.marker.data(), w.stream.data(), nc, w.rx.data(), n_streams, 0.002, -INFINITY, INFINITY, solver,
                       flags, min_rx, 0, weight, grid, 0, o.fixes.data(), o.aux.data(), cap < 0 ? (int)o.fixes.size() : cap, &o.nf, ms.data(),
                       mt.data(), member_cap < 0 ? nc : member_cap, &o.nm, heads.data(), &nh);
}
}  // namespace

int main() {
  for (long long nc : {1ll, 2ll, 3ll, 5ll, 6ll, 63ll, 64ll, 65ll, 255ll, 256ll, 257ll, 1023ll, 1024ll, 1025ll, 65536ll, 1000003ll})
    for (long long ns : {1ll, 10ll, 11ll, 1024ll}) {
      const mh::RuleLayout L = mh::layout_rule((size_t)nc, (size_t)ns);
      expect(L.bytes % 256 == 0 && L.aux + ((size_t)nc / 3 + 1) * mh::kAuxBytes <= L.bytes && L.member_ts + (size_t)nc * 8 <= L.aux &&
                 L.fixes + ((size_t)nc / 3 + 1) * mh::kFixBytes <= L.member_stream && L.rx + (size_t)ns * 24 <= L.fixes && L.w + (size_t)nc * 4 <= L.cnt &&
                 L.bytes >= mh::layout((size_t)nc, (size_t)ns).bytes,
             "layout_rule");
    }
  double p[3];
  Out o;
  {  // six receivers, the damped rule with the restart, behind 300 foreign entries; two grids
    World w;
    place(w, 6, p);
    for (int k = 0; k < 300; ++k) w.add(1000.0 + k * 1e-9, 0x100000u + (unsigned)k, 5 - k % 2, 19, 0);
    for (int s = 0; s < 6; ++s) w.add(arrival(w, s, p, 1000.0 + 1e-4), 7u, s, 19, 0);
    w.sort_from(300);
    for (int grid : {1, 3}) {
      expect(run(w, 6, 1, 1, 4, 1.0, grid, o) == 0 && o.nf == 1 && o.nm == 6, "six: one group");
      expect(o.fixes[0].n_rx == 6 && o.fixes[0].icao == 7 && o.aux[0].alt_ft == -1 && o.aux[0].tries >= o.fixes[0].iters && o.aux[0].reserved == 0,
             "six: the rows");
    }
    expect(run(w, 6, 0, 0, 4, 1.0, 0, o) == 0 && o.nf == 1 && o.aux[0].alt_ft == -1 && o.aux[0].tries == 0, "six: _GN");
    expect(run(w, 6, 1, 1, 3, 1.0, 0, o) == -22 && run(w, 6, 0, 1, 4, 1.0, 0, o) == -22 && run(w, 6, 1, 2, 3, 0.0, 0, o) == -22 && run(w, 6, 2, 0, 4, 1.0, 0, o) == -22,
           "the argument table");
  }
  {  // three hearings with an altitude, three without, four without: the aided three and the four are rows
    World w;
    place(w, 7, p);
    for (int s = 0; s < 3; ++s) w.add(arrival(w, s, p, 1000.0), 1u, s, 11, 30000);
    for (int s = 0; s < 3; ++s) w.add(arrival(w, s, p, 1000.01), 2u, s, 19, 30000);
    for (int s = 3; s < 7; ++s) w.add(arrival(w, s, p, 1000.02), 3u, s, 8, 30000);
    w.sort_from(0);
    expect(run(w, 7, 1, 3, 3, 1.0, 2, o) == 0 && o.nf == 2 && o.nm == 7, "3+4: two rows");
    expect(o.fixes[0].n_rx == 3 && o.aux[0].alt_ft == 30000 && (o.aux[0].flags & 1u) && o.fixes[1].n_rx == 4 && o.fixes[1].first == 3 &&
               o.aux[1].alt_ft == -1,
           "3+4: the rows");
    expect(run(w, 7, 1, 3, 3, 1.0, 0, o, 1, 7) == -28 && o.nf == 2 && o.nm == 7 && run(w, 7, 1, 3, 3, 1.0, 0, o, 2, 6) == -28, "3+4: -ENOSPC");
    expect(run(w, 7, 1, 1, 4, 1.0, 0, o) == 0 && o.nf == 1 && o.nm == 4, "3+4: without the flag only the four");
  }
  {  // 65 hearings of one reply at one instant by 65 streams, and four streams at one point
    World w;
    place(w, 65, p);
    for (int s = 0; s < 65; ++s) w.add(1000.5, 9u, s, 12, 1000);
    expect(run(w, 65, 1, 3, 3, 0.5, 0, o) == 0 && o.nf == 1 && o.nm == 64 && o.fixes[0].n_heard == 65 && o.aux[0].alt_ft == 1000, "cap: 64 of 65");
    World one;
    for (int s = 0; s < 4; ++s) { one.rx.push_back(6378137.0); one.rx.push_back(0.0); one.rx.push_back(0.0); one.add(1000.0, 5u, s, 19, 0); }
    expect(run(one, 4, 1, 1, 4, 1.0, 0, o) == 0 && o.nf == 1 && o.fixes[0].status == ml::kSingular && o.aux[0].flags == 2u, "singular");
  }
  printf(failures ? "mlat_rule_sanitize: %d failures\n" : "mlat_rule_sanitize: ok\n", failures);
  return failures != 0;
}
