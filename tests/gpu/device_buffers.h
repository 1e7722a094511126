// device_buffers.h -- TEST INFRASTRUCTURE ONLY.  What tests/gpu/shared_device_driver.hip and tests/gpu/dedup_device_driver.hip
// share: parts in device memory with a guard tail behind each, the way they come back whole after a launch group, and the
// sticky first HIP error (tests/gpu/mlat_device_driver.hip's g_dead rule).  Host code only.  Never linked into libadsb_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <initializer_list>
#include <vector>

namespace {
constexpr unsigned char kGuard = 0xA5;
constexpr size_t kTail = 256;

int g_dead = 0;                                       // the first HIP error's code: nothing is queued after it

// the status of one HIP call -> 0, or the sticky code -1000 - hipError_t
int hip_rc(hipError_t e) {
  if (e != hipSuccess && !g_dead) g_dead = -1000 - (int)e;
  return g_dead;
}
#define HIP_OR_RETURN(call) do { if (hip_rc(call)) return g_dead; } while (0)

// `bytes` a kernel may touch and kTail guard bytes behind them, in device memory; everything starts as the guard byte, then
// `src` (if any) is copied to the front.  read_only: the part must come back equal to src.
struct Part {
  void* p = nullptr;
  size_t bytes = 0;
  const void* src = nullptr;
  bool read_only = false;
  std::vector<unsigned char> host;                    // the part as back() last saw it, tail included
  Part() = default;
  Part(const Part&) = delete;
  Part& operator=(const Part&) = delete;
  ~Part() { if (p && !g_dead) (void)hipFree(p); }

  int make(const void* src_, size_t bytes_, bool read_only_) {
    src = src_; bytes = bytes_; read_only = read_only_ && src_ != nullptr;
    host.assign(bytes + kTail, kGuard);
    HIP_OR_RETURN(hipMalloc(&p, bytes + kTail));
    HIP_OR_RETURN(hipMemset(p, kGuard, bytes + kTail));
    if (src && bytes) HIP_OR_RETURN(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    return 0;
  }
  template <class T> T* as() const { return (T*)p; }
  template <class T> const T* got() const { return (const T*)host.data(); }
  // the part back whole -> 0; -1: a guard byte, or a byte of a read-only part, has changed; or the sticky HIP code
  int back() {
    HIP_OR_RETURN(hipMemcpy(host.data(), p, host.size(), hipMemcpyDeviceToHost));
    for (size_t k = bytes; k < host.size(); ++k)
      if (host[k] != kGuard) return -1;
    if (read_only && bytes && memcmp(host.data(), src, bytes) != 0) return -1;
    return 0;
  }
  bool equals(const void* want) const { return bytes == 0 || memcmp(host.data(), want, bytes) == 0; }
};

// after a launch group: the launches' status, the null stream drained, then every part back whole -> 0, -1, or a HIP code
int group_end(int launched, std::initializer_list<Part*> parts) {
  HIP_OR_RETURN((hipError_t)launched);
  HIP_OR_RETURN(hipDeviceSynchronize());
  int rc = 0;
  for (Part* q : parts) {
    const int r = q->back();
    if (g_dead) return g_dead;
    if (r) rc = r;
  }
  HIP_OR_RETURN(hipGetLastError());
  return rc;
}
}  // namespace
