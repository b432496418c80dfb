// What the integer map kernels share (froc.hip, evalmask.hip, rank.hip, mining.hip): wave and workgroup scans, the per-wave vote count
// and the dword reads of a flat byte map.  256 threads = 4 waves of 64, thread order.  Integer arithmetic only: no order reaches a result.
// (The training kernels' helpers are common.hpp's; the floating-point reductions stay with their kernels, their order reaches the bits.)
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace sslcr {

// the sum over the wave's 64 lanes of an integer, by a butterfly; every lane must be active
template <class T>
__device__ __forceinline__ typename std::enable_if<std::is_integral<T>::value, T>::type wave_sum(T v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);                   // bound: 6 steps; every lane ends with the total
  return v;
}

// inclusive sum / max over the wave's 64 lanes, in lane order; every lane must be active
__device__ __forceinline__ int wave_incl_sum(int v) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {                // bound: 6 steps
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}
__device__ __forceinline__ int wave_incl_max(int v) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {                // bound: 6 steps
    const int u = __shfl_up(v, d);
    if (lane >= d) v = max(v, u);
  }
  return v;
}

// exclusive sum over the workgroup's 256 values in thread order; *total = the sum over all; sh: 4 ints.  All 256 threads must reach
// the call (two barriers, and the shuffles read every lane): no caller returns or diverges before it.
__device__ __forceinline__ int block_excl_sum(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int incl = wave_incl_sum(v);
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  int off = 0, all = 0;
  for (int k = 0; k < 4; ++k) {
    all += sh[k];
    if (k < w) off += sh[k];
  }
  *total = all;
  __syncthreads();
  return off + incl - v;
}

// exclusive max-scan over the workgroup's 256 values, in thread order (reverse = false: thread t gets the max over the threads before
// it) or in reverse thread order (the max over the threads after it); nothing before = none, a value below every input; *total = the
// max over all; sh: 4 ints.  All 256 threads must reach the call.  The forward branch is wave_incl_max's loop, kept inline: through
// the helper edt_rows_kernel and the three AUC kernels come out with other code (tools/device_code_diff.sh).
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

// *counter += the number of the wave's lanes that vote: one integer atomic per wave (none where nobody votes), by lane 0; every lane
// must be active
template <class T>
__device__ __forceinline__ void wave_vote_add(T* counter, bool vote) {
  const unsigned long long votes = __ballot(vote);
  if (votes && (threadIdx.x & 63) == 0) atomicAdd(counter, (T)__popcll(votes));
}

// the four bytes of the aligned dword at flat address addr (a multiple of 4) of a byte map of n cells; bytes past the end of the
// array read as "not there": the last, partial dword is read bytewise, none past the end
__device__ __forceinline__ unsigned mask_dword(const unsigned char* mask, int64_t addr, int64_t n) {
  if (addr + 4 <= n) return *reinterpret_cast<const unsigned*>(mask + addr);
  unsigned v = 0;
  for (int j = 0; j < 4; ++j)
    if (addr + j < n) v |= (unsigned)mask[addr + j] << (8 * j);
  return v;
}

}  // namespace sslcr
