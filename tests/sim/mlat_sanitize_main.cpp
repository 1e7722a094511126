// mlat_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program around mlat_driver.cpp for AddressSanitizer and
// UndefinedBehaviorSanitizer on the CPU (tools/mlat_sanitize.sh): adsb_mlat.h's sizing rule over the sizes at which a part's
// length crosses a 256-byte boundary, and two of tests/test_mlat.py's cases through the emulated kernels -- a head that is the
// last thread of a workgroup with its members on the far side, behind a tile and more of foreign entries, and 65 hearings of
// one reply (the cap of 64 candidates).  Exit status 0: every call returned what it should.
#include "mlat_driver.cpp"

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
  void add(double t, unsigned id, int mk, int s) {
    ts.push_back(t); marker.push_back(mk); stream.push_back(s);
    unsigned char b[14] = {0x8D, (unsigned char)(id >> 16), (unsigned char)(id >> 8), (unsigned char)id, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    bits.insert(bits.end(), b, b + 14);
  }
};

// n receivers on a 200 km circle around (4e6, 0, 5e6) with alternating heights, and an aircraft 9 km above its middle
void place(World& w, int n, double p[3]) {
  for (int s = 0; s < n; ++s) {
    const double a = 6.283185307179586 * s / n;
    w.rx.push_back(4.0e6 + 1.0e5 * std::cos(a) - 800.0 * (s % 3));
    w.rx.push_back(1.0e5 * std::sin(a));
    w.rx.push_back(5.0e6 + 1200.0 * (s % 2));
  }
  p[0] = 4.0e6 + 7000.0; p[1] = 12000.0; p[2] = 5.0e6 + 9000.0;
}

int run(World& w, int n_streams, int grid, int* n_fixes, int* n_members, std::vector<ml::Fix>& fixes) {
  const int nc = (int)w.ts.size();
  fixes.assign((size_t)nc / 4 + 1, ml::Fix());
  std::vector<int> ms((size_t)nc + 1), heads((size_t)nc + 1);
  std::vector<double> mt((size_t)nc + 1);
  int nh = 0;
  return sim_mlat(w.ts.data(), w.bits.data(), w.marker.data(), w.stream.data(), nc, w.rx.data(), n_streams, 0.002, -INFINITY, INFINITY, 4, grid, 0,
                  fixes.data(), (int)fixes.size(), n_fixes, ms.data(), mt.data(), nc, n_members, heads.data(), &nh);
}
}  // namespace

int main() {
  // the sizing rule
  for (long long nc : {1ll, 63ll, 64ll, 65ll, 255ll, 256ll, 257ll, 1023ll, 1024ll, 1025ll, 65536ll, 1000003ll})
    for (long long ns : {1ll, 10ll, 11ll, 1024ll}) {
      const mh::Layout L = mh::layout((size_t)nc, (size_t)ns);
      expect(L.bytes % 256 == 0 && L.member_ts + (size_t)nc * 8 <= L.bytes && L.fixes + ((size_t)nc / 4 + 1) * mh::kFixBytes <= L.member_stream &&
                 L.rx + (size_t)ns * 24 <= L.fixes && L.w + (size_t)nc * 4 <= L.cnt,
             "layout");
    }
  double p[3];
  {  // a head as entry 255 + 1024: its workgroup's last thread, a tile and more of foreign entries in front of it
    World w;
    place(w, 6, p);
    const int front = 255 + 1024;
    for (int k = 0; k < front; ++k) w.add(1000.0 + k * 1e-9, 0x100000u + (unsigned)k, 2, 5 - k % 2);
    for (int s = 0; s < 6; ++s) {
      const double dx = p[0] - w.rx[3 * s], dy = p[1] - w.rx[3 * s + 1], dz = p[2] - w.rx[3 * s + 2];
      w.add(1000.0 + 1e-4 + std::sqrt(dx * dx + dy * dy + dz * dz) / ml::kC, 7u, 2, s);
    }
    // (the carry is time-sorted: the six arrivals come behind the fillers; sort them among themselves)
    for (size_t i = (size_t)front; i < w.ts.size(); ++i)
      for (size_t j = i + 1; j < w.ts.size(); ++j)
        if (w.ts[j] < w.ts[i]) { std::swap(w.ts[i], w.ts[j]); std::swap(w.stream[i], w.stream[j]); }
    int nf = 0, nm = 0;
    std::vector<ml::Fix> fixes;
    for (int grid : {1, 3}) {
      expect(run(w, 6, grid, &nf, &nm, fixes) == 0 && nf == 1 && nm == 6, "seam: one group of six");
      expect(fixes[0].n_rx == 6 && fixes[0].n_heard == 6 && fixes[0].icao == 7 && fixes[0].first == 0, "seam: the fix's counts");
    }
  }
  {  // 65 hearings of one reply at one instant by 65 streams: 64 candidates, n_heard 65
    World w;
    place(w, 65, p);
    for (int s = 0; s < 65; ++s) w.add(1000.5, 9u, 2, s);
    int nf = 0, nm = 0;
    std::vector<ml::Fix> fixes;
    expect(run(w, 65, 0, &nf, &nm, fixes) == 0 && nf == 1 && nm == 64, "cap: one group");
    expect(fixes[0].n_rx == 64 && fixes[0].n_heard == 65, "cap: 64 of 65");
    // ... and no room for it
    std::vector<int> ms(8), heads(80);
    std::vector<double> mt(8);
    int nh = 0;
    expect(sim_mlat(w.ts.data(), w.bits.data(), w.marker.data(), w.stream.data(), 65, w.rx.data(), 65, 0.002, -INFINITY, INFINITY, 4, 0, 0, fixes.data(), 1,
                    &nf, ms.data(), mt.data(), 8, &nm, heads.data(), &nh) == -28 && nf == 1 && nm == 64, "cap: -ENOSPC states the counts");
  }
  printf(failures ? "mlat_sanitize: %d failures\n" : "mlat_sanitize: ok\n", failures);
  return failures != 0;
}
