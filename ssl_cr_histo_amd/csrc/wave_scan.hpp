// Integer wave and workgroup scans the map kernels share (evalmask.hip, rank.hip): 256 threads = 4 waves of 64, thread order.
#pragma once
#include <hip/hip_runtime.h>

namespace sslcr {

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);                   // bound: 6 steps; every lane ends with the total
  return v;
}

// exclusive max-scan over the workgroup's 256 values, in thread order (reverse = false: thread t gets the max over the threads before
// it) or in reverse thread order (the max over the threads after it); nothing before = none, a value below every input; *total = the
// max over all; sh: 4 ints
__device__ __forceinline__ int block_scan_max(int v, bool reverse, int none, int* sh, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {                // bound: 6 steps
    const int u = reverse ? __shfl_down(v, d) : __shfl_up(v, d);
    if (reverse ? lane + d < 64 : lane >= d) v = max(v, u);
  }
  if (lane == (reverse ? 0 : 63)) sh[w] = v;        // the wave's total
  int ex = reverse ? __shfl_down(v, 1) : __shfl_up(v, 1);
  if (lane == (reverse ? 63 : 0)) ex = none;
  __syncthreads();
  int all = none;
  for (int k = 0; k < 4; ++k) {
    all = max(all, sh[k]);
    if (reverse ? k > w : k < w) ex = max(ex, sh[k]);
  }
  *total = all;
  __syncthreads();
  return ex;
}

}  // namespace sslcr
