// softfec_device_driver.hip -- TEST INFRASTRUCTURE ONLY.  Runs the soft-decision CRC repair's kernels ON THE DEVICE through the
// shipped launchers of gr_adsb_amd/csrc/adsb_softfec.hip (compiled beside this file as the library compiles it:
// tests/device_build.py), every buffer in device memory with a guard tail behind it (device_buffers.h).  The entry points have
// the signatures of the emulator driver tests/sim/softfec_driver.cpp, so that tests/test_gpu_softfec_device.py runs the cases of
// tests/test_softfec.py unchanged.  -> 0, -1 (a guard byte or a read-only part changed) or -1000 - hipError_t (sticky).
#include "device_buffers.h"

#include "../../gr_adsb_amd/csrc/adsb_softfec.h"

extern "C" {

int sim_soft_records(int mode, const void* data, long long n, long long origin, float scale, int sps, const void* rule,
                     unsigned long long* recs, int n_kept, int out_cap, unsigned long long* mirror, int mirror_cap, unsigned long long* rows,
                     int grid) {
  if (g_dead) return g_dead;
  const size_t sample = mode == 0 ? 8 : mode <= 2 ? 4 : 2, rec = adsb_softfec_host::kRecWords * 8, row = adsb_softfec_host::kRowBytes;
  if (!mirror) mirror_cap = 0;
  Part d_data, d_recs, d_mirror, d_rows, d_n;
  if (d_data.make(data, (size_t)n * sample, true) || d_recs.make(recs, (size_t)out_cap * rec, false) ||
      d_mirror.make(mirror, (size_t)mirror_cap * rec, false) || d_rows.make(rows, (size_t)out_cap * row, false) ||
      d_n.make(&n_kept, sizeof(int), true))
    return g_dead;
  const int e = adsb_softfec_host::launch_records(nullptr, (unsigned)grid, mode, d_data.p, n, origin, scale, sps, rule, d_recs.p, d_n.as<int>(),
                                                  out_cap, mirror ? d_mirror.p : nullptr, mirror_cap, d_rows.p);
  const int rc = group_end(e, {&d_data, &d_recs, &d_mirror, &d_rows, &d_n});
  if (rc) return rc;
  memcpy(recs, d_recs.host.data(), (size_t)out_cap * rec);
  if (mirror_cap) memcpy(mirror, d_mirror.host.data(), (size_t)mirror_cap * rec);
  memcpy(rows, d_rows.host.data(), (size_t)out_cap * row);
  return 0;
}

int sim_soft_slices(const float* data, long long n, const long long* tag_idx, int sps, const void* rule, unsigned char* bits14,
                    unsigned char* ok, int ntags, unsigned long long* rows, int grid) {
  if (g_dead) return g_dead;
  Part d_data, d_tags, d_bits, d_ok, d_rows;
  if (d_data.make(data, (size_t)n * 4, true) || d_tags.make(tag_idx, (size_t)ntags * 8, true) || d_bits.make(bits14, (size_t)ntags * 14, false) ||
      d_ok.make(ok, (size_t)ntags, false) || d_rows.make(rows, (size_t)ntags * adsb_softfec_host::kRowBytes, false))
    return g_dead;
  const int e = adsb_softfec_host::launch_slices(nullptr, (unsigned)grid, d_data.p, n, d_tags.as<long long>(), sps, rule, d_bits.as<unsigned char>(),
                                                 d_ok.as<unsigned char>(), ntags, d_rows.p);
  const int rc = group_end(e, {&d_data, &d_tags, &d_bits, &d_ok, &d_rows});
  if (rc) return rc;
  memcpy(bits14, d_bits.host.data(), (size_t)ntags * 14);
  memcpy(ok, d_ok.host.data(), (size_t)ntags);
  memcpy(rows, d_rows.host.data(), (size_t)ntags * adsb_softfec_host::kRowBytes);
  return 0;
}
}
