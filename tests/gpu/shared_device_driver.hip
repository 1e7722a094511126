// shared_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  The time order's kernels on the GPU, over the SHIPPED translation unit
// gr_adsb_amd/csrc/adsb_shared.hip -- compiled as a unit of its own with the library's flags and linked beside this file into
// tests/gpu/libadsb_shared_dev.so (tests/test_gpu_shared_device.py builds it) -- and its real launchers launch_keys /
// launch_sort / launch_gather / launch_scatter with their own cover() and blocks().  This file launches no k_shared_* kernel
// itself and includes no device code.  Its entries:
//
//   sim_shared_sort, sim_shared_sort_keys   tests/sim/shared_driver.cpp's entries of the same names, argument for argument: the
//                                           stable pair sort alone.  The keys of sim_shared_sort are made on the host by
//                                           host_time_key, the map adsb_shared_device.h states (dev_shared_chain holds the
//                                           device's own map to the same statement in NumPy).
//   dev_shared_chain                        launch_keys -> launch_sort -> launch_gather -> launch_scatter on stated records,
//                                           first[], start[], fs and stated "sorted rows" (what the decode step would leave).
//
// Every array lives in device memory as a part of its own (device_buffers.h): filled with the guard byte first, a guard tail
// behind it.  After each launcher all parts come back whole: a changed guard byte, or a changed byte of an input the kernels
// only read, is -1.  Every HIP call's status is checked: an error is -1000 - hipError_t, no further GPU call is made, and every
// later call of this library returns the same code at once (dev_shared_dead).  Never linked into libadsb_hip.so.
#include "device_buffers.h"

#include "../../gr_adsb_amd/csrc/adsb_shared.h"

namespace shh = adsb_shared_host;

static_assert(shh::kRecBytes == 32 && shh::kRowBytes == 72 && shh::kSortTile == 4096, "the sizes adsb_shared.h states");

namespace {
// adsb_shared_device.h's time_key, restated for the host: a set sign bit flips every bit, a clear one sets it; -0.0 is +0.0
unsigned long long host_time_key(double ts) {
  unsigned long long b;
  memcpy(&b, &ts, 8);
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the stable pair sort alone on keys0 / vals0 [n] -> keys_out / vals_out [n] (either may be null).  0, -1, or a HIP code
int sort_pairs(const unsigned long long* keys0, const unsigned* vals0, int n, unsigned long long* keys_out, unsigned* vals_out) {
  if (g_dead) return g_dead;
  const size_t nn = (size_t)n;
  Part keys, vals, keys_tmp, vals_tmp, hist;
  if (keys.make(keys0, nn * 8, false) || vals.make(vals0, nn * 4, false) || keys_tmp.make(nullptr, nn * 8, false) ||
      vals_tmp.make(nullptr, nn * 4, false) || hist.make(nullptr, shh::sort_hist_bytes(n), false))
    return g_dead;
  const int rc = group_end(shh::launch_sort(nullptr, keys.as<unsigned long long>(), vals.as<unsigned>(), keys_tmp.as<unsigned long long>(),
                                            vals_tmp.as<unsigned>(), n, hist.as<unsigned>()),
                           {&keys, &vals, &keys_tmp, &vals_tmp, &hist});
  if (rc) return rc;
  if (keys_out) memcpy(keys_out, keys.host.data(), nn * 8);
  if (vals_out) memcpy(vals_out, vals.host.data(), nn * 4);
  return 0;
}
}  // namespace

extern "C" {

int dev_shared_dead() { return g_dead; }
int sim_shared_sort_tile() { return shh::kSortTile; }

int sim_shared_sort(const double* ts, const unsigned* vals0, int n, unsigned* order_out, unsigned long long* keys_out) {
  if (n <= 0) return 0;
  std::vector<unsigned long long> keys((size_t)n);
  std::vector<unsigned> vals((size_t)n);
  for (int i = 0; i < n; ++i) { keys[(size_t)i] = host_time_key(ts[i]); vals[(size_t)i] = vals0 ? vals0[i] : (unsigned)i; }
  return sort_pairs(keys.data(), vals.data(), n, keys_out, order_out);
}

int sim_shared_sort_keys(const unsigned long long* keys0, int n, unsigned* order_out) {
  if (n <= 0) return 0;
  std::vector<unsigned long long> sorted((size_t)n);
  std::vector<unsigned> vals((size_t)n);
  for (int i = 0; i < n; ++i) vals[(size_t)i] = (unsigned)i;
  const int r = sort_pairs(keys0, vals.data(), n, sorted.data(), order_out);
  if (r) return r;
  for (int i = 1; i < n; ++i)
    if (sorted[(size_t)i - 1] > sorted[(size_t)i]) return -2;
  return 0;
}

// The chain.  In: recs[n][4] (the call's list; word 0 the offset), first[n_items + 1], start[n_items], fs; sorted_rows[n][9]: the
// rows of the time-ordered list; delivered[n][4]: the records k_shared_scatter writes word 3 into, at list positions.
// Out: ts_out[n] and keys_out[n] as k_shared_keys leaves them (list positions), order_out[n], srecs_out[n][4] and sts_out[n]
// (k_shared_gather), recs_out[n][4] and rows_out[n][9] (k_shared_scatter).
// 0; -1: a guard byte or a read-only input was overwritten; -2: the sorted values are no permutation, or k_shared_keys' values
// are not 0 .. n-1; -5: a bad argument; <= -1000: a HIP status.
int dev_shared_chain(const unsigned long long* recs_in, int n, const int* first, const double* start, int n_items, double fs,
                     const unsigned long long* sorted_rows, const unsigned long long* delivered, double* ts_out, unsigned long long* keys_out,
                     int* order_out, unsigned long long* srecs_out, double* sts_out, unsigned long long* recs_out, unsigned long long* rows_out) {
  if (n < 0) return -5;
  if (n == 0) return 0;
  if (n_items <= 0 || first[0] != 0 || first[n_items] != n || !(fs > 0)) return -5;
  for (int i = 0; i < n_items; ++i)
    if (first[i] > first[i + 1]) return -5;
  if (g_dead) return g_dead;
  const size_t nn = (size_t)n, rec = shh::kRecBytes, row = shh::kRowBytes;
  Part recs, fst, st0, keys, vals, ts, keys_tmp, vals_tmp, hist, srecs, sts, order, srows, out_recs, out_rows;
  if (recs.make(recs_in, nn * rec, true) || fst.make(first, ((size_t)n_items + 1) * 4, true) || st0.make(start, (size_t)n_items * 8, true) ||
      keys.make(nullptr, nn * 8, false) || vals.make(nullptr, nn * 4, false) || ts.make(nullptr, nn * 8, false) ||
      keys_tmp.make(nullptr, nn * 8, false) || vals_tmp.make(nullptr, nn * 4, false) || hist.make(nullptr, shh::sort_hist_bytes(n), false) ||
      srecs.make(nullptr, nn * rec, false) || sts.make(nullptr, nn * 8, false) || order.make(nullptr, nn * 4, false) ||
      srows.make(sorted_rows, nn * row, true) || out_recs.make(delivered, nn * rec, false) || out_rows.make(nullptr, nn * row, false))
    return g_dead;
  const hipStream_t st = nullptr;
  const auto all = {&recs, &fst, &st0, &keys, &vals, &ts, &keys_tmp, &vals_tmp, &hist, &srecs, &sts, &order, &srows, &out_recs, &out_rows};
  int rc;

  if ((rc = group_end(shh::launch_keys(st, recs.p, n, fst.as<int>(), st0.as<double>(), n_items, fs, keys.as<unsigned long long>(),
                                       vals.as<unsigned>(), ts.as<double>()), all)))
    return rc;
  memcpy(ts_out, ts.host.data(), nn * 8);
  memcpy(keys_out, keys.host.data(), nn * 8);
  for (size_t i = 0; i < nn; ++i)
    if (vals.got<unsigned>()[i] != (unsigned)i) return -2;

  if ((rc = group_end(shh::launch_sort(st, keys.as<unsigned long long>(), vals.as<unsigned>(), keys_tmp.as<unsigned long long>(),
                                       vals_tmp.as<unsigned>(), n, hist.as<unsigned>()), all)))
    return rc;
  if (!ts.equals(ts_out)) return -1;
  {
    std::vector<char> hit(nn, 0);
    for (size_t k = 0; k < nn; ++k) {
      const unsigned t = vals.got<unsigned>()[k];
      if (t >= (unsigned)n || hit[t]) return -2;                     // (k_shared_gather would skip it, k_shared_scatter too)
      hit[t] = 1;
    }
  }
  std::vector<unsigned> sorted_vals(vals.got<unsigned>(), vals.got<unsigned>() + nn);

  if ((rc = group_end(shh::launch_gather(st, recs.p, ts.as<double>(), vals.as<unsigned>(), n, srecs.p, sts.as<double>(), order.as<int>()), all)))
    return rc;
  if (!ts.equals(ts_out) || !vals.equals(sorted_vals.data())) return -1;
  memcpy(order_out, order.host.data(), nn * 4);
  memcpy(srecs_out, srecs.host.data(), nn * rec);
  memcpy(sts_out, sts.host.data(), nn * 8);

  if ((rc = group_end(shh::launch_scatter(st, srecs.p, srows.p, order.as<int>(), n, out_recs.p, out_rows.p), all))) return rc;
  if (!order.equals(order_out) || !srecs.equals(srecs_out) || !sts.equals(sts_out)) return -1;
  memcpy(recs_out, out_recs.host.data(), nn * rec);
  memcpy(rows_out, out_rows.host.data(), nn * row);
  return 0;
}
}
