// hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.  What a shipped translation unit's `#include <hip/hip_runtime.h>` finds when
// tests/sim/mlat_track_driver.cpp compiles that unit with g++ for the SIMT emulator (-I tests/sim/hipstub): hipsim.h, and just
// enough of the launch interface that the unit's own launchers -- their cover(), their order, their arguments -- run
// unchanged, each kernel on hipsim::launch.  The dynamic-LDS and stream arguments are accepted and unused.  Never on hipcc's
// include path; never linked into libadsb_hip.so.
#pragma once
#include "../../hipsim.h"

struct dim3 {
  unsigned x;
  explicit dim3(unsigned v) : x(v) {}
};
typedef void* hipStream_t;
inline int hipGetLastError() { return 0; }
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
  do { (void)(stream); hipsim::launch(kernel, (grid).x, (block).x, __VA_ARGS__); } while (0)

inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, sizeof r); return r; }
inline double __longlong_as_double(long long v) { double r; memcpy(&r, &v, sizeof r); return r; }
