// softmax of one row of logits, one thread per row: the ONE place this quotient is formed.  heads.hip (softmax_col_kernel,
// predict_kernel) and tta.hip (predict_tta_kernel) include it, so that a probability has the same bits whichever entry wrote it.
// And what the two predict kernels share besides: torch.argmax's step, and the confusion matrix counted per workgroup -- 32-bit
// integer atomics on cells in LDS (a workgroup adds at most 256 per cell), flushed with one 64-bit integer atomic per non-empty cell:
// exact, order-independent, the caller's int64 matrix accumulates across calls (annotation.hip's map_confusion_kernel takes the flush).
#pragma once
#include "common.hpp"

namespace sslcr {

// softmax(l[0..C-1])[col] with the row's max m and sum s = sum_c expf(l[c] - m)
__device__ __forceinline__ void softmax_row_stats(const float* l, int C, float& m, float& s) {
  m = l[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(l[c] - m);
}
__device__ __forceinline__ float softmax_value(const float* l, int col, float m, float s) { return expf(l[col] - m) / s; }

constexpr int CONFUSION_MAX_C = 64;                 // cells: unsigned[CONFUSION_MAX_C * CONFUSION_MAX_C]; C <= 64 is the entries' rule

// cells[0 .. count) = 0, then a barrier: all 256 threads must reach the call (as for confusion_flush)
__device__ __forceinline__ void confusion_clear(unsigned* cells, int count) {
  for (int k = threadIdx.x; k < count; k += 256) cells[k] = 0u;
  __syncthreads();
}
// one row with target y and prediction b; a target outside [0, C) counts nowhere
__device__ __forceinline__ void confusion_count(unsigned* cells, int C, int64_t y, int b) {
  if (y >= 0 && y < C) atomicAdd(&cells[(int)y * C + b], 1u);
}
// cell k of the workgroup into cell k of the caller's matrix, if it counted anything
__device__ __forceinline__ void confusion_flush_cell(const unsigned* cells, int k, int64_t* confusion) {
  if (cells[k]) atomicAdd(reinterpret_cast<unsigned long long*>(confusion) + k, (unsigned long long)cells[k]);
}
// a barrier, then every cell of [0, count)
__device__ __forceinline__ void confusion_flush(const unsigned* cells, int count, int64_t* confusion) {
  __syncthreads();
  for (int k = threadIdx.x; k < count; k += 256) confusion_flush_cell(cells, k, confusion);
}
// torch.argmax's step for the key at index c, above every index seen so far (best at index b): the lowest index of the maximum, a
// NaN is the maximum -- once best is a NaN it stays, so the lowest NaN index wins
__device__ __forceinline__ void argmax_step(float& best, int& b, float key, int c) {
  if (best == best && (key > best || key != key)) { best = key; b = c; }
}

}  // namespace sslcr
