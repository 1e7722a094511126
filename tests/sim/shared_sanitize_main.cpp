// shared_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program around tests/sim/shared_driver.cpp for
// AddressSanitizer + UndefinedBehaviorSanitizer (tools/shared_sanitize.sh): the pair sort at the sizes around a wavefront and a
// tile, and one partition of tests/golden/g_shared.npz from a job file that tools/shared_sanitize_job.py writes (the calls'
// lists and, from the plain-Python replay, the flags, rows and order to expect).  Nothing here is loaded into python.
//   job file, little endian: int32 n_streams, fec, all; double fs; double start[n_streams]; int32 n_calls; per call:
//   int32 n, n_items; int32 item_stream[n_items]; int32 item_first[n_items + 1]; u8 bits[n][14]; int64 offset[n];
//   u16 flags[n] (ADSB_BURST_AP_KNOWN | _AP_FEC alone); u8 rows[n][72]; int32 order[n]
#include "shared_driver.cpp"

#include <cstdio>
#include <random>

namespace {
bool read(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int sort_checks() {
  std::mt19937_64 rng(1);
  for (int n : {1, 63, 64, 65, 4095, 4096, 4097, 3 * sh::kSortTile + 1}) {
    std::vector<double> ts((size_t)n);
    for (double& t : ts) t = (double)((long long)(rng() % 41) - 20) * ((rng() & 1) ? 1.0 : 1760000000.25);
    std::vector<unsigned> order((size_t)n);
    std::vector<unsigned long long> keys((size_t)n);
    if (sim_shared_sort(ts.data(), nullptr, n, order.data(), keys.data()) != 0) return 1;
    for (int i = 1; i < n; ++i) {
      const double a = ts[order[(size_t)i - 1]], b = ts[order[(size_t)i]];
      if (a > b || (a == b && order[(size_t)i - 1] > order[(size_t)i])) { fprintf(stderr, "sort: n %d, place %d\n", n, i); return 1; }
    }
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (sort_checks()) return 1;
  if (argc < 2) { fprintf(stderr, "usage: %s JOB\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int head[3];
  double fs;
  if (!read(f, head, sizeof head) || !read(f, &fs, sizeof fs)) return 2;
  std::vector<double> start((size_t)head[0]);
  int n_calls = 0;
  if (!read(f, start.data(), start.size() * 8) || !read(f, &n_calls, 4)) return 2;
  void* h = sim_shared_open(head[0], 0, head[1], head[2], 1, fs);
  for (int s = 0; s < head[0]; ++s) sim_shared_set_start(h, s, start[(size_t)s]);
  long long total = 0;
  for (int c = 0; c < n_calls; ++c) {
    int n = 0, n_items = 0;
    if (!read(f, &n, 4) || !read(f, &n_items, 4)) return 2;
    std::vector<int> ist((size_t)n_items), first((size_t)n_items + 1), order((size_t)n), got_order((size_t)n);
    std::vector<unsigned char> bits((size_t)n * 14), rows((size_t)n * 72), got_rows((size_t)n * 72);
    std::vector<long long> off((size_t)n);
    std::vector<unsigned short> flags((size_t)n), got_flags((size_t)n);
    std::vector<double> ts((size_t)n);
    if (!read(f, ist.data(), ist.size() * 4) || !read(f, first.data(), first.size() * 4) || !read(f, bits.data(), bits.size()) ||
        !read(f, off.data(), off.size() * 8) || !read(f, flags.data(), flags.size() * 2) || !read(f, rows.data(), rows.size()) ||
        !read(f, order.data(), order.size() * 4))
      return 2;
    const int rc = sim_shared_call(h, bits.data(), off.data(), nullptr, n, ist.data(), first.data(), n_items, 1 + c % 3, got_flags.data(),
                                   got_rows.data(), got_order.data(), ts.data());
    if (rc) { fprintf(stderr, "call %d: driver returned %d\n", c, rc); return 1; }
    for (int t = 0; t < n; ++t)
      if ((got_flags[(size_t)t] & 0xCu) != flags[(size_t)t] || got_order[(size_t)t] != order[(size_t)t] ||
          memcmp(&got_rows[(size_t)t * 72], &rows[(size_t)t * 72], 72) != 0) {
        fprintf(stderr, "call %d, position %d differs from the replay\n", c, t);
        return 1;
      }
    total += n;
  }
  fclose(f);
  long long planes, cap, grows, used;
  sim_shared_stats(h, &planes, &cap, &grows, &used);
  long long removed = sim_shared_expire(h, 1760000030, 2);   // the rehash with ages, too
  sim_shared_close(h);
  printf("shared decoder under the sanitizers: %d calls, %lld records, %lld planes, %lld growths, %lld expired: ok\n", n_calls, total,
         planes, grows, removed);
  return total > 0 ? 0 : 1;
}
