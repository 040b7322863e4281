// launch.h -- the launch macro of the kernel translation units: HIP-event profiling hooks around every launch; and what
// launchers ask of the runtime or size the same way in more than one place
#pragma once
#include <map>
#include <mutex>
#include <tuple>
#include "dispatch.h"
#include "kernels.h"
static inline void prof_begin(LaunchCtx* P, const char* name) {
  if(P -> prof_begin) P -> prof_begin(P -> prof_user, name, P -> stream);
}
static inline void prof_end(LaunchCtx* P) {
  if(P -> prof_end) P -> prof_end(P -> prof_user, P -> stream);
}
#define LAUNCH(name, kern, grid, block, lds, ...)                                    \
  do {                                                                               \
    prof_begin(P, name);                                                             \
    hipLaunchKernelGGL(kern, grid, block, lds, P -> stream, __VA_ARGS__);            \
    prof_end(P);                                                                     \
    hipError_t e_ = hipGetLastError();                                               \
    if(e_ != hipSuccess) return (int)e_;                                             \
  } while(0)

// Workgroups of `kernel` that the device keeps resident at this block size and LDS use (its register and LDS use
// decide); 0 when the runtime cannot tell.  Asked once per (kernel, block size, LDS bytes).
static inline int resident_blocks(const void* kernel, int block, size_t lds) {
  static std::mutex mx; static std::map<std::tuple<const void*, int, size_t>, int> cache;
  std::lock_guard<std::mutex> lock(mx);
  const auto key = std::make_tuple(kernel, block, lds);
  auto it = cache.find(key);
  if(it != cache.end()) return it -> second;
  int per_cu = 0, dev = 0, cus = 0;
  if(hipOccupancyMaxActiveBlocksPerMultiprocessor(& per_cu, kernel, block, lds) != hipSuccess) { per_cu = 0; (void)hipGetLastError(); }
  if(hipGetDevice(& dev) != hipSuccess || hipDeviceGetAttribute(& cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { cus = 0; (void)hipGetLastError(); }
  return cache[key] = per_cu * cus;
}
// A launch with more than 64 KB of dynamic LDS fails unless the kernel was opted in to that many bytes.  Not part of
// LAUNCH: a launcher that never opted in keeps failing above 64 KB rather than changing what it accepts unnoticed.
static inline hipError_t lds_opt_in(const void* kernel, size_t bytes) {
  if(bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// LDS bytes of the paired noise filter (noise_filter_pair: two frames in one N-point transform): the N points, N / 2
// twiddles, the N / 2 + 1 bins of both PSDs and npsd staged target rows as float2, 16 floats of reduction, `extra` bytes
// of the caller's own
static inline size_t nf_pair_lds(int N, int npsd, size_t extra = 0) {
  const size_t lds = (size_t)(N + N / 2 + N / 2 + 1 + npsd) * sizeof(float2) + 16 * sizeof(float) + extra;
  return (lds + 15) / 16 * 16;
}
