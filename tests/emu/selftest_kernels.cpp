// TEST INFRASTRUCTURE ONLY -- kernels that are wrong on purpose (and their correct versions), to show that the schedules of
// hipemu.cpp detect what they are there to detect (tests/test_emu_schedules.py).  Plain C++ over the stand-in header: never
// compiled for a GPU, not part of pycwt_amd/.  256 threads, one LDS array of integers; thread t of workgroup b writes
// value(b, t) and reads a neighbour's element: out[256 b + t] is what it found.
#include <hip/hip_runtime.h>

namespace {
constexpr int kThreads = 256;

inline int value(int salt, int b, int t) { return salt + 1000 * b + t; }
inline void wave_sync() { __builtin_amdgcn_wave_barrier(); }

// 1: a dependence BETWEEN waves behind a wave barrier (wrong on the hardware; lockstep cannot see it)
void k_selftest_cross_wave(int salt, int* out) {
  HIP_DYNAMIC_SHARED(int, lds)
  const int t = threadIdx.x, b = blockIdx.x;
  lds[t] = value(salt, b, t);
  wave_sync();
  out[kThreads * b + t] = lds[t ^ 64];
}
void k_selftest_cross_wave_ok(int salt, int* out) {
  HIP_DYNAMIC_SHARED(int, lds)
  const int t = threadIdx.x, b = blockIdx.x;
  lds[t] = value(salt, b, t);
  __syncthreads();
  out[kThreads * b + t] = lds[t ^ 64];
}
// 2: an upward dependence on no barrier at all
void k_selftest_up(int salt, int* out) {
  HIP_DYNAMIC_SHARED(int, lds)
  const int t = threadIdx.x, b = blockIdx.x;
  lds[t] = value(salt, b, t);
  out[kThreads * b + t] = lds[t + 1 < kThreads ? t + 1 : t];
}
// 3: a downward dependence on no barrier at all (thread order hides it)
void k_selftest_down(int salt, int* out) {
  HIP_DYNAMIC_SHARED(int, lds)
  const int t = threadIdx.x, b = blockIdx.x;
  lds[t] = value(salt, b, t);
  out[kThreads * b + t] = lds[t > 0 ? t - 1 : t];
}
// 2 and 3 inside one wave: the wave barrier suffices
void k_selftest_up_ok(int salt, int* out) {
  HIP_DYNAMIC_SHARED(int, lds)
  const int t = threadIdx.x, b = blockIdx.x;
  lds[t] = value(salt, b, t);
  wave_sync();
  out[kThreads * b + t] = lds[(t & ~63) | ((t + 1) & 63)];
}
void k_selftest_down_ok(int salt, int* out) {
  HIP_DYNAMIC_SHARED(int, lds)
  const int t = threadIdx.x, b = blockIdx.x;
  lds[t] = value(salt, b, t);
  wave_sync();
  out[kThreads * b + t] = lds[(t & ~63) | ((t + 63) & 63)];
}
}  // namespace

// which: 0 cross_wave, 1 cross_wave_ok, 2 up, 3 up_ok, 4 down, 5 down_ok.  out: 256 * blocks ints.  Returns 0, or -1 for an
// unknown kernel.
extern "C" int hipemu_selftest(int which, int blocks, int salt, int* out) {
  const dim3 grid(blocks), block(kThreads);
  const size_t lds = kThreads * sizeof(int);
  switch (which) {
    case 0: hipLaunchKernelGGL(k_selftest_cross_wave, grid, block, lds, nullptr, salt, out); return 0;
    case 1: hipLaunchKernelGGL(k_selftest_cross_wave_ok, grid, block, lds, nullptr, salt, out); return 0;
    case 2: hipLaunchKernelGGL(k_selftest_up, grid, block, lds, nullptr, salt, out); return 0;
    case 3: hipLaunchKernelGGL(k_selftest_up_ok, grid, block, lds, nullptr, salt, out); return 0;
    case 4: hipLaunchKernelGGL(k_selftest_down, grid, block, lds, nullptr, salt, out); return 0;
    case 5: hipLaunchKernelGGL(k_selftest_down_ok, grid, block, lds, nullptr, salt, out); return 0;
  }
  return -1;
}
