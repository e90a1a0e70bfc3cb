// Host stand-ins for the few HIP names csrc/resample.hip uses, so that the file's kernels and launchers compile and run as an
// ordinary C++ program (tests/test_resample_emu_host.py): a workgroup is 256 threads with a barrier, its LDS an exact-size heap block
// (the address sanitizer then sees every index), workgroups run one after the other.  Test infrastructure only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#include <pthread.h>
#include "mi355asr.h"
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct Idx { int x, y, z; };
inline thread_local Idx threadIdx, blockIdx;
inline float* g_lds;
inline pthread_barrier_t g_bar;
inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
typedef void* hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0, hipMemcpyHostToDevice = 1, hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return 0; }
inline const char* hipGetErrorString(int) { return "x"; }
inline char g_err[512];
inline int fail(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); return code; }
#define HIP_TRY(expr) do { if ((expr) != 0) return fail(MI355ASR_EHIP, "hip"); } while (0)
inline void emu_launch(const std::function<void()>& fn, dim3 grid, dim3 block, size_t ldsb) {
  for (unsigned by = 0; by < grid.y; ++by)
    for (unsigned bx = 0; bx < grid.x; ++bx) {
      g_lds = (float*)aligned_alloc(16, (ldsb + 15) & ~(size_t)15);
      pthread_barrier_init(&g_bar, nullptr, block.x);
      std::vector<std::thread> th;
      for (unsigned t = 0; t < block.x; ++t)
        th.emplace_back([&, t]() { threadIdx = Idx{(int)t, 0, 0}; blockIdx = Idx{(int)bx, (int)by, 0}; fn(); });
      for (auto& x : th) x.join();
      pthread_barrier_destroy(&g_bar);
      free(g_lds);
    }
}
#define hipLaunchKernelGGL(k, grid, block, ldsb, s, ...) emu_launch([&]() { k(__VA_ARGS__); }, grid, block, ldsb)
