// adsb_env_hip.h -- the HIP device environment adsb_device.h is written against (see its head comment): the product's
// versions of adsb_wave_sync / adsb_uniform / adsb_readlane / adsb_above4 / adsb_mag2 / adsb_fmax3 / the DPP wave primitives /
// adsb_bitrep32 / adsb_sdot4 / adsb_cold, with inline assembly and DPP for gfx950.  Included by adsb_hip.hip right before
// adsb_device.h, and by tests/gpu/detect_units_driver.hip, which runs each of them on the device against a plain definition.
// Needs <hip/hip_runtime.h>.
#pragma once

// wavefront-level ordering point used by adsb_device.h: LDS traffic of one wavefront is executed in
// program order by the hardware, this only stops the compiler from moving LDS accesses across it
__device__ __forceinline__ void adsb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int adsb_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int adsb_readlane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
// `v`, made to depend on `after` without an instruction: whatever uses the result cannot be scheduled before `after` exists
__device__ __forceinline__ unsigned adsb_after(unsigned v, float after) {
  asm volatile("" : "+v"(v) : "v"(after));
  return v;
}
// the value itself, but opaque to the optimiser (per-lane: a vector register)
__device__ __forceinline__ int adsb_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
// c + the sum of the four products of the signed bytes of a and b (v_dot4c_i32_i8)
__device__ __forceinline__ int adsb_sdot4(int a, int b, int c) { return __builtin_amdgcn_sdot4(a, b, c, false); }
// streamed single-use data: non-temporal load (every sample is fetched exactly once)
template <class Q>
__device__ __forceinline__ Q adsb_ld_stream(const char* p) {
  using V = float __attribute__((ext_vector_type(sizeof(Q) / 4)));
  return __builtin_bit_cast(Q, __builtin_nontemporal_load(reinterpret_cast<const V*>(p)));
}
// issue priority of the calling wavefront among the wavefronts of its SIMD (0 = default ... 3)
template <int P>
__device__ __forceinline__ void adsb_setprio() { __builtin_amdgcn_s_setprio(P); }
// written once, read once much later (k_detect's burst lists): non-temporal store
typedef unsigned long long adsb_u64x2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ void adsb_st_stream(T* p, T v) { __builtin_nontemporal_store(v, p); }
// acc = 16*acc + the four threshold bits (x >= thr, NaN -> 0) of a, b, c, d (a highest): four compares into four
// scalar pairs, then a chain of add-with-carry (acc = 2*acc + bit).  Batched by four because gfx950 wants two wait
// states between a vector instruction that writes a scalar pair and a vector instruction that reads it: the three
// other compares are that distance, no s_nop is spent.
__device__ __forceinline__ unsigned adsb_above4(unsigned acc, float a, float b, float c, float d, float thr) {
  unsigned long long ca, cb, cc, cd;
  asm("v_cmp_le_f32 %1, %6, %7\n\t"
      "v_cmp_le_f32 %2, %6, %8\n\t"
      "v_cmp_le_f32 %3, %6, %9\n\t"
      "v_cmp_le_f32 %4, %6, %10\n\t"
      "v_addc_co_u32 %0, vcc, %5, %5, %1\n\t"
      "v_addc_co_u32 %0, vcc, %0, %0, %2\n\t"
      "v_addc_co_u32 %0, vcc, %0, %0, %3\n\t"
      "v_addc_co_u32 %0, vcc, %0, %0, %4"
      : "=&v"(acc), "=&s"(ca), "=&s"(cb), "=&s"(cc), "=&s"(cd)
      : "v"(acc), "s"(thr), "v"(a), "v"(b), "v"(c), "v"(d)
      : "vcc");
  return acc;
}
// x*x + y*y with two rounded products and one rounded add: one packed multiply on the register pair the
// sample was loaded into, one add.  As asm statements because the compiler's own packing of re*re + im*im wants (re0, re1) /
// (im0, im1) pairs and pays for them with three or four register moves per 16-byte load.
__device__ __forceinline__ float adsb_mag2(float x, float y) {
  typedef float v2f __attribute__((ext_vector_type(2)));
  v2f a = {x, y}, r;
  float m;
  asm("v_pk_mul_f32 %0, %1, %1" : "=v"(r) : "v"(a));
  asm("v_add_f32 %0, %1, %2" : "=v"(m) : "v"(r.x), "v"(r.y));
  return m;
}
// maximum of three floats with the hardware's own NaN rule (a quiet NaN operand is skipped); as an asm statement so that
// no canonicalising instruction is spent on operands that come straight from memory
__device__ __forceinline__ float adsb_fmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// the value of the lane below (lane 0: `fill`): DPP wave_shr:1
__device__ __forceinline__ unsigned adsb_lane_up1(unsigned v, unsigned fill) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xF, 0xF, false);
}
// inclusive prefix sum over the 64 lanes: four row_shr steps inside each row of 16, then row_bcast:15 / row_bcast:31
__device__ __forceinline__ unsigned adsb_wave_incl_scan(unsigned x) {
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
  return x;
}
// minimum over the 64 lanes (wave-uniform result), same DPP ladder
__device__ __forceinline__ unsigned adsb_wave_min_u32(unsigned v) {
#define ADSB_MIN_STEP(ctrl, rows)                                                                  \
  {                                                                                                \
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, ctrl, rows, 0xF, false);  \
    v = o < v ? o : v;                                                                             \
  }
  ADSB_MIN_STEP(0x111, 0xF) ADSB_MIN_STEP(0x112, 0xF) ADSB_MIN_STEP(0x114, 0xF) ADSB_MIN_STEP(0x118, 0xF)
  ADSB_MIN_STEP(0x142, 0xA) ADSB_MIN_STEP(0x143, 0xC)
#undef ADSB_MIN_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// maximum over the 64 lanes (wave-uniform result)
__device__ __forceinline__ unsigned adsb_wave_max_u32(unsigned v) {
#define ADSB_MAX_STEP(ctrl, rows)                                                                 \
  {                                                                                                \
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xF, false);   \
    v = o > v ? o : v;                                                                             \
  }
  ADSB_MAX_STEP(0x111, 0xF) ADSB_MAX_STEP(0x112, 0xF) ADSB_MAX_STEP(0x114, 0xF) ADSB_MAX_STEP(0x118, 0xF)
  ADSB_MAX_STEP(0x142, 0xA) ADSB_MAX_STEP(0x143, 0xC)
#undef ADSB_MAX_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// the dynamic LDS of the launch as an int array
#define ADSB_DYN_LDS_INT(name) extern __shared__ int name[]
// workgroup-local (LDS) address space qualifier for pointers that crossed a function call as generic pointers
#define ADSB_LDS __attribute__((address_space(3)))
// bit i of x -> bits 2i and 2i+1 (scalar unit; the argument must be wave-uniform)
__device__ __forceinline__ unsigned long long adsb_bitrep32(unsigned x) {
  unsigned long long r;
  asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(r) : "s"(x));
  return r;
}

// The kernel's own argument block in (kernarg) memory: DetectArgs is the FIRST parameter of every kernel that runs
// detect_body, so the block starts with it.  Through an empty asm statement, so that loads through it are neither hoisted
// out of the tile loop nor merged with the by-value copy: a field read through this pointer costs one s_load where it is
// used and no scalar register anywhere else.
namespace adsb { struct DetectArgs; }
typedef const __attribute__((address_space(4))) adsb::DetectArgs* adsb_cold_ptr;
__device__ __forceinline__ adsb_cold_ptr adsb_cold(const adsb::DetectArgs&) {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (adsb_cold_ptr)p;
}
// The same for an argument block that lies in a device TABLE (k_batch: one entry per workgroup, the entry's address is
// wave-uniform).  The table is not written while the kernel runs, so its entries may be read through the constant address
// space like the kernel-argument segment: scalar loads where a field is used, and cold() keeps its type.
__device__ __forceinline__ adsb_cold_ptr adsb_cold_at(const adsb::DetectArgs* e) {
  unsigned long long p = (unsigned long long)e;
  asm volatile("" : "+s"(p));
  return (adsb_cold_ptr)p;
}
#define ADSB_COLD_AT(e) adsb_cold_at(e)
