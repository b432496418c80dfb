// softmax of one row of logits, one thread per row: the ONE place this quotient is formed.  heads.hip (softmax_col_kernel,
// predict_kernel) and tta.hip (predict_tta_kernel) include it, so that a probability has the same bits whichever entry wrote it.
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

}  // namespace sslcr
