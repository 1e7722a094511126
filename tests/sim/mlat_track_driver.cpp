// mlat_track_driver.cpp -- TEST INFRASTRUCTURE ONLY.  The MLAT track store's kernels (gr_adsb_amd/csrc/adsb_mlat_track_device.h)
// AND their real launchers on the SIMT emulator: the shipped translation units adsb_mlat_track.hip and adsb_shared.hip (its
// launch_sort is the store's key sort) are included as they stand, compiled by g++ with tests/sim/hipstub in front of the
// include path, where <hip/hip_runtime.h> is hipsim.h plus a hipLaunchKernelGGL that runs each launch on hipsim::launch -- so
// cover(), the launch order and every argument are the library's own.  The host's rule of adsb_hip.hip is restated in
// mlat_track_host_rule.h, which tests/gpu/mlat_track_device_driver.hip shares; here a Part is host memory.  Fed synthetic fix and
// aux arrays directly.  The host's own code runs only in tests/test_gpu_mlat_track.py.  Never linked into libadsb_hip.so.
#include "../../gr_adsb_amd/csrc/adsb_shared.hip"
#include "../../gr_adsb_amd/csrc/adsb_mlat_track.hip"

#include "mlat_track_host_rule.h"

namespace th = adsb_mlat_track_host;

namespace {
constexpr size_t kTail = 256;

// tests/gpu/device_buffers.h's Part, in host memory
struct Part {
  void* p = nullptr;
  size_t bytes = 0;
  const void* src = nullptr;
  bool read_only = false;
  std::vector<unsigned char> host;                    // the part itself, tail included
  int make(const void* src_, size_t bytes_, bool read_only_) {
    src = src_; bytes = bytes_; read_only = read_only_ && src_ != nullptr;
    host.assign(bytes + kTail, track_rule::kGuardByte);
    if (src && bytes) memcpy(host.data(), src, bytes);
    p = host.data();
    return 0;
  }
  int back() const {
    for (size_t k = bytes; k < host.size(); ++k)
      if (host[k] != track_rule::kGuardByte) return -1;
    return read_only && bytes && memcmp(host.data(), src, bytes) != 0 ? -1 : 0;
  }
};

int end(int launched, std::initializer_list<Part*> parts) {
  if (launched) return -1000 - launched;
  int rc = 0;
  for (Part* q : parts) if (q->back()) rc = -1;
  return rc;
}
}  // namespace

extern "C" {

int sim_track_row_bytes() { return (int)sizeof(adsb_mlat_track::Track); }
int sim_track_rule_bytes() { return (int)sizeof(adsb_mlat_track::Rule); }
int sim_track_sort_tile() { return adsb_shared_host::kSortTile; }
// layout(n): the 14 parts' offsets in carve()'s order -> offs[14]; returns the total
unsigned long long sim_track_layout(long long n, unsigned long long* offs) {
  const th::Layout L = th::layout((size_t)n);
  const size_t at[14] = {L.cnts, L.stats, L.w, L.cnt, L.sel, L.run_start, L.run_len, L.pos, L.newidx, L.keys, L.keys_tmp, L.vals, L.vals_tmp, L.hist};
  if (offs) for (int k = 0; k < 14; ++k) offs[k] = at[k];
  return (unsigned long long)L.bytes;
}
unsigned sim_track_cover(long long work, int per) { return th::cover(work, per); }

int sim_track_update(const void* fixes, const void* aux, int ng, const void* rule, const void* store, int nt, void* store_out, int* nt_out,
                     long long* stats) {
  return track_rule::update<Part>(end, fixes, aux, ng, rule, store, nt, store_out, nt_out, stats);
}
int sim_track_read(const void* store, int nt, int min_fixes, double cutoff, void* rows, int cap, int* n) {
  return track_rule::read<Part>(end, store, nt, min_fixes, cutoff, false, rows, cap, n);
}
int sim_track_expire(const void* store, int nt, double cutoff, void* store_out, int* nt_out) {
  return track_rule::read<Part>(end, store, nt, 0, cutoff, true, store_out, 0, nt_out);
}
}
