// detect_units_driver.hip -- TEST INFRASTRUCTURE ONLY.  Single functions of gr_adsb_amd/csrc/adsb_device.h, and the product's
// device environment they are written against (gr_adsb_amd/csrc/adsb_env_hip.h: inline assembly and DPP), on the MI355X by
// themselves: the entry points of tests/sim/sim_driver.cpp's last section, with the same signatures, on device memory.  Built
// by tests/test_gpu_units.py with the library's flags; never linked into libadsb_hip.so.
//
// Every kernel runs 256 threads and a bounded grid-stride loop; every argument is range-checked on the host before a launch;
// every output buffer has kGuard words behind it that must come back untouched (dev_units_guard_bad counts the ones that did
// not).  After a failed HIP call nothing more is launched (dev_units_dead).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_env_hip.h"

#include "../../gr_adsb_amd/csrc/adsb_device.h"

using namespace adsb;

namespace {

constexpr int kUnitThreads = 256, kUnitWaves = kUnitThreads / 64;
constexpr int kMaxGrid = 1024;
constexpr int kMaxChain = 8;               // windows per chain
constexpr size_t kGuard = 64;              // 32-bit words behind every output buffer
constexpr unsigned kGuardWord = 0xA5C3F00Du;

int g_dead = 0;                            // the first HIP error (or -22: arguments out of range); no launch after it
long long g_guard_bad = 0;                 // guard words found changed, over all calls

#define UNITS_TRY(call)                                                                            \
  do {                                                                                             \
    const hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                        \
      if (!g_dead) g_dead = (int)e_;                                                               \
      fprintf(stderr, "detect_units_driver: %s: %s\n", #call, hipGetErrorString(e_));              \
      return;                                                                                      \
    }                                                                                              \
  } while (0)

// device copy of a host input
struct In {
  void* p = nullptr;
  In(const void* h, size_t bytes) {
    if (g_dead) return;
    UNITS_TRY(hipMalloc(&p, bytes ? bytes : 4));
    if (bytes) UNITS_TRY(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
  }
  ~In() { if (p) (void)hipFree(p); }
  In(const In&) = delete;
  template <class T> const T* as() const { return (const T*)p; }
};
// device buffer for a host output: starts as the host buffer does, guard words behind it
struct Out {
  void* p = nullptr;
  void* host;
  size_t bytes;
  Out(void* h, size_t nbytes) : host(h), bytes(nbytes) {
    if (g_dead) return;
    UNITS_TRY(hipMalloc(&p, bytes + kGuard * 4));
    if (bytes) UNITS_TRY(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    std::vector<unsigned> g(kGuard, kGuardWord);
    UNITS_TRY(hipMemcpy((char*)p + bytes, g.data(), kGuard * 4, hipMemcpyHostToDevice));
  }
  void fetch() {
    if (g_dead || !p) return;
    std::vector<unsigned> g(kGuard, 0u);
    UNITS_TRY(hipMemcpy(g.data(), (char*)p + bytes, kGuard * 4, hipMemcpyDeviceToHost));
    for (unsigned v : g) if (v != kGuardWord) ++g_guard_bad;
    if (bytes) UNITS_TRY(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost));
  }
  ~Out() { if (p) (void)hipFree(p); }
  Out(const Out&) = delete;
  template <class T> T* as() const { return (T*)p; }
};

void finish() {
  if (g_dead) return;
  UNITS_TRY(hipGetLastError());
  UNITS_TRY(hipDeviceSynchronize());
}

int grid_for(long long items, int per_block) {
  long long g = (items + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

__device__ __forceinline__ int unit_wave() { return adsb_uniform((int)(blockIdx.x * kUnitWaves + (threadIdx.x >> 6))); }
__device__ __forceinline__ int unit_wave_stride() { return (int)gridDim.x * kUnitWaves; }

// one wavefront per chain, all 64 lanes active: v0 / v1 / val0 / val1 exactly as burst_from_window forms them
template <bool QUANT>
__global__ __launch_bounds__(kUnitThreads) void k_unit_median(const float* windows, const int* nwin, const int* chain_start,
                                                              const unsigned* hint0, int n_chains, int total, unsigned* med_out,
                                                              unsigned* hint_out) {
  const int lane = threadIdx.x & 63;
  for (int c = unit_wave(); c < n_chains; c += unit_wave_stride()) {
    unsigned hint = (unsigned)adsb_uniform((int)hint0[c]);
    int w0 = adsb_uniform(chain_start[c]), w1 = adsb_uniform(chain_start[c + 1]);
    if (w0 < 0) w0 = 0;
    if (w1 > total) w1 = total;
    if (w1 > w0 + kMaxChain) w1 = w0 + kMaxChain;
    for (int w = w0; w < w1; ++w) {
      int n = adsb_uniform(nwin[w]);
      n = n < 0 ? 0 : n > 128 ? 128 : n;
      const bool val0 = lane < n, val1 = lane + 64 < n;
      const float v0 = val0 ? windows[(size_t)w * 128 + lane] : 0.0f;
      const float v1 = val1 ? windows[(size_t)w * 128 + lane + 64] : 0.0f;
      const float med = noise_median<QUANT>(n, val0, val1, v0, v1, hint);
      if (lane == 0) {
        med_out[w] = __builtin_bit_cast(unsigned, med);
        hint_out[w] = hint;
      }
    }
  }
}

// one thread per row of taps: tp[k * h], h floats apart
template <int HALF, bool RAW>
__global__ __launch_bounds__(kUnitThreads) void k_unit_chips(const float* buf, int row_floats, int h, int n, unsigned char* out) {
  for (int i = (int)(blockIdx.x * kUnitThreads + threadIdx.x); i < n; i += (int)gridDim.x * kUnitThreads)
    out[i] = chips_match<HALF, RAW>(buf + (size_t)i * row_floats, h) ? 1 : 0;
}

// body_convert over 16-byte loads: one thread per load, words[4 k .. 4 k + 4) -> out[8 k .. 8 k + 8)
template <int MODE>
__global__ __launch_bounds__(kUnitThreads) void k_unit_convert(const unsigned* words, long long nloads, float scale, float* out) {
  for (long long k = (long long)blockIdx.x * kUnitThreads + threadIdx.x; k < nloads; k += (long long)gridDim.x * kUnitThreads) {
    const float4 q = reinterpret_cast<const float4*>(words)[k];
    float m[8];
    body_convert<MODE>(q, scale, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[8 * k + j] = m[j];
  }
}

// the wave primitives: one wavefront per row of 64 lanes, every lane's result stored
__global__ __launch_bounds__(kUnitThreads) void k_unit_min_max(const unsigned* in, int rows, unsigned* mn, unsigned* mx) {
  const int lane = threadIdx.x & 63;
  for (int r = unit_wave(); r < rows; r += unit_wave_stride()) {
    const unsigned v = in[(size_t)r * 64 + lane];
    mn[(size_t)r * 64 + lane] = adsb_wave_min_u32(v);
    mx[(size_t)r * 64 + lane] = adsb_wave_max_u32(v);
  }
}
__global__ __launch_bounds__(kUnitThreads) void k_unit_scan(const unsigned* in, int rows, unsigned* out) {
  const int lane = threadIdx.x & 63;
  for (int r = unit_wave(); r < rows; r += unit_wave_stride()) out[(size_t)r * 64 + lane] = adsb_wave_incl_scan(in[(size_t)r * 64 + lane]);
}
__global__ __launch_bounds__(kUnitThreads) void k_unit_lane_up1(const unsigned* in, const unsigned* fill, int rows, unsigned* out) {
  const int lane = threadIdx.x & 63;
  for (int r = unit_wave(); r < rows; r += unit_wave_stride()) out[(size_t)r * 64 + lane] = adsb_lane_up1(in[(size_t)r * 64 + lane], fill[r]);
}
__global__ __launch_bounds__(kUnitThreads) void k_unit_above4(const unsigned* acc, const float* x, const float* thr, int rows,
                                                              unsigned* out) {
  const int lane = threadIdx.x & 63;
  for (int r = unit_wave(); r < rows; r += unit_wave_stride()) {
    const size_t i = (size_t)r * 64 + lane;
    const float t = __builtin_bit_cast(float, adsb_uniform(__builtin_bit_cast(int, thr[r])));      // a scalar operand
    out[i] = adsb_above4(acc[i], x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], t);
  }
}
// the argument is wave-uniform: one wavefront per value, lane 0 stores
__global__ __launch_bounds__(kUnitThreads) void k_unit_bitrep32(const unsigned* x, int n, unsigned long long* out) {
  for (int i = unit_wave(); i < n; i += unit_wave_stride()) {
    const unsigned long long r = adsb_bitrep32((unsigned)adsb_uniform((int)x[i]));
    if ((threadIdx.x & 63) == 0) out[i] = r;
  }
}
__global__ __launch_bounds__(kUnitThreads) void k_unit_mag2(const float* x, const float* y, long long n, float* out) {
  for (long long i = (long long)blockIdx.x * kUnitThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kUnitThreads)
    out[i] = adsb_mag2(x[i], y[i]);
}

template <int HALF>
void chips_launch(int raw, const In& buf, int row_floats, int h, int n, Out& out) {
  const int grid = grid_for(n, kUnitThreads);
  if (raw) k_unit_chips<HALF, true><<<grid, kUnitThreads>>>(buf.as<float>(), row_floats, h, n, out.as<unsigned char>());
  else k_unit_chips<HALF, false><<<grid, kUnitThreads>>>(buf.as<float>(), row_floats, h, n, out.as<unsigned char>());
}

}  // namespace

extern "C" {

int dev_units_dead() { return g_dead; }
long long dev_units_guard_bad() { return g_guard_bad; }
int sim_median_path_count() { return kMedianPathCount; }

// path_out is the emulator's alone (ADSB_MEDIAN_PATH is empty in a device build): not touched
void sim_noise_median(int quant, const float* windows, const int* nwin, const int* chain_start, const unsigned* hint0,
                      int n_chains, unsigned* med_out, unsigned* hint_out, unsigned* /*path_out*/) {
  if (g_dead || n_chains <= 0) return;
  const int total = chain_start[n_chains];
  bool ok = chain_start[0] == 0 && total >= 0;
  for (int c = 0; ok && c < n_chains; ++c) {
    const int len = chain_start[c + 1] - chain_start[c];
    ok = len >= 0 && len <= kMaxChain;
  }
  for (int w = 0; ok && w < total; ++w) ok = nwin[w] >= 0 && nwin[w] <= 128;
  if (!ok) { g_dead = -22; return; }
  In d_win(windows, (size_t)total * 128 * 4), d_nwin(nwin, (size_t)total * 4), d_start(chain_start, (size_t)(n_chains + 1) * 4),
      d_hint0(hint0, (size_t)n_chains * 4);
  Out d_med(med_out, (size_t)total * 4), d_hint(hint_out, (size_t)total * 4);
  if (g_dead) return;
  const int grid = grid_for(n_chains, kUnitWaves);
  if (quant)
    k_unit_median<true><<<grid, kUnitThreads>>>(d_win.as<float>(), d_nwin.as<int>(), d_start.as<int>(), d_hint0.as<unsigned>(),
                                                n_chains, total, d_med.as<unsigned>(), d_hint.as<unsigned>());
  else
    k_unit_median<false><<<grid, kUnitThreads>>>(d_win.as<float>(), d_nwin.as<int>(), d_start.as<int>(), d_hint0.as<unsigned>(),
                                                 n_chains, total, d_med.as<unsigned>(), d_hint.as<unsigned>());
  finish();
  d_med.fetch();
  d_hint.fetch();
}

// half = 1, 2, 4, 10: that instance; half < 0: the run-time instance at -half samples per chip.  The taps are laid out at
// their stride, every float between them is +inf.  raw = 0: the instance for computed samples, whose taps must hold no
// signalling NaN
int sim_chips_match(int half, int raw, const float* taps, int n, unsigned char* out) {
  const int h = half < 0 ? -half : half;
  if (!((half == 1 || half == 2 || half == 4 || half == 10) || (half < 0 && half >= -64)) || n < 0) return -1;
  if (g_dead || n == 0) return g_dead ? -2 : 0;
  const int row_floats = 15 * h + 1;
  std::vector<float> buf((size_t)n * row_floats, INFINITY);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 16; ++k) buf[(size_t)i * row_floats + (size_t)k * h] = taps[(size_t)i * 16 + k];
  In d_buf(buf.data(), buf.size() * 4);
  Out d_out(out, (size_t)n);
  if (g_dead) return -2;
  if (half == 1) chips_launch<1>(raw, d_buf, row_floats, h, n, d_out);
  else if (half == 2) chips_launch<2>(raw, d_buf, row_floats, h, n, d_out);
  else if (half == 4) chips_launch<4>(raw, d_buf, row_floats, h, n, d_out);
  else if (half == 10) chips_launch<10>(raw, d_buf, row_floats, h, n, d_out);
  else chips_launch<0>(raw, d_buf, row_floats, h, n, d_out);
  finish();
  d_out.fetch();
  return g_dead ? -2 : 0;
}

// mode 3 int8, 4 offset-binary uint8, 5 / 6 their power-of-two-scale instances; nwords % 4 == 0 is used, a remainder is ignored
void sim_convert8(int mode, const unsigned* words, long long nwords, float scale, float* out) {
  const long long nloads = nwords / 4;
  if (g_dead || nloads <= 0) return;
  if (mode < 3 || mode > 6) { g_dead = -22; return; }
  In d_words(words, (size_t)nloads * 16);
  Out d_out(out, (size_t)nloads * 32);
  if (g_dead) return;
  const int grid = grid_for(nloads, kUnitThreads);
  if (mode == 3) k_unit_convert<3><<<grid, kUnitThreads>>>(d_words.as<unsigned>(), nloads, scale, d_out.as<float>());
  else if (mode == 4) k_unit_convert<4><<<grid, kUnitThreads>>>(d_words.as<unsigned>(), nloads, scale, d_out.as<float>());
  else if (mode == 5) k_unit_convert<kModeSc8Pow2><<<grid, kUnitThreads>>>(d_words.as<unsigned>(), nloads, scale, d_out.as<float>());
  else k_unit_convert<kModeCu8Pow2><<<grid, kUnitThreads>>>(d_words.as<unsigned>(), nloads, scale, d_out.as<float>());
  finish();
  d_out.fetch();
}

void sim_wave_min_max(const unsigned* in, int rows, unsigned* mn, unsigned* mx) {
  if (g_dead || rows <= 0) return;
  In d_in(in, (size_t)rows * 256);
  Out d_mn(mn, (size_t)rows * 256), d_mx(mx, (size_t)rows * 256);
  if (g_dead) return;
  k_unit_min_max<<<grid_for(rows, kUnitWaves), kUnitThreads>>>(d_in.as<unsigned>(), rows, d_mn.as<unsigned>(), d_mx.as<unsigned>());
  finish();
  d_mn.fetch();
  d_mx.fetch();
}

void sim_wave_incl_scan(const unsigned* in, int rows, unsigned* out) {
  if (g_dead || rows <= 0) return;
  In d_in(in, (size_t)rows * 256);
  Out d_out(out, (size_t)rows * 256);
  if (g_dead) return;
  k_unit_scan<<<grid_for(rows, kUnitWaves), kUnitThreads>>>(d_in.as<unsigned>(), rows, d_out.as<unsigned>());
  finish();
  d_out.fetch();
}

void sim_lane_up1(const unsigned* in, const unsigned* fill, int rows, unsigned* out) {
  if (g_dead || rows <= 0) return;
  In d_in(in, (size_t)rows * 256), d_fill(fill, (size_t)rows * 4);
  Out d_out(out, (size_t)rows * 256);
  if (g_dead) return;
  k_unit_lane_up1<<<grid_for(rows, kUnitWaves), kUnitThreads>>>(d_in.as<unsigned>(), d_fill.as<unsigned>(), rows, d_out.as<unsigned>());
  finish();
  d_out.fetch();
}

void sim_above4(const unsigned* acc, const float* x, const float* thr, int rows, unsigned* out) {
  if (g_dead || rows <= 0) return;
  In d_acc(acc, (size_t)rows * 256), d_x(x, (size_t)rows * 1024), d_thr(thr, (size_t)rows * 4);
  Out d_out(out, (size_t)rows * 256);
  if (g_dead) return;
  k_unit_above4<<<grid_for(rows, kUnitWaves), kUnitThreads>>>(d_acc.as<unsigned>(), d_x.as<float>(), d_thr.as<float>(), rows,
                                                                d_out.as<unsigned>());
  finish();
  d_out.fetch();
}

void sim_bitrep32(const unsigned* x, int n, unsigned long long* out) {
  if (g_dead || n <= 0) return;
  In d_x(x, (size_t)n * 4);
  Out d_out(out, (size_t)n * 8);
  if (g_dead) return;
  k_unit_bitrep32<<<grid_for(n, kUnitWaves), kUnitThreads>>>(d_x.as<unsigned>(), n, d_out.as<unsigned long long>());
  finish();
  d_out.fetch();
}

void sim_mag2(const float* x, const float* y, long long n, float* out) {
  if (g_dead || n <= 0) return;
  In d_x(x, (size_t)n * 4), d_y(y, (size_t)n * 4);
  Out d_out(out, (size_t)n * 4);
  if (g_dead) return;
  k_unit_mag2<<<grid_for(n, kUnitThreads), kUnitThreads>>>(d_x.as<float>(), d_y.as<float>(), n, d_out.as<float>());
  finish();
  d_out.fetch();
}

}  // extern "C"
