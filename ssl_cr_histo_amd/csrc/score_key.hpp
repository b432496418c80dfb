// The order-preserving integer key of a float32 score: the ONE definition rank.hip (rank_keys_kernel) and knn.hip (the top-k lists)
// share, so that "greater" means the same to the ROC-AUC counts and to the k-NN selection.  A score is its bit pattern b; the
// unsigned order of the keys is the order of the scores under float compares, with -0 tied to +0.  NaNs have no place in that order:
// each caller states what it does with them (rank.hip counts them and leaves them out, knn.hip ranks them below every number).
#pragma once
#include <stdint.h>

namespace sslcr {

__host__ __device__ __forceinline__ bool score_is_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
__host__ __device__ __forceinline__ uint32_t score_key(uint32_t b) {
  if ((b << 1) == 0u) b = 0u;                       // -0 ties with +0
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
// the bits of the score a key came from (a -0 comes back as +0)
__host__ __device__ __forceinline__ uint32_t score_from_key(uint32_t key) { return (key >> 31) ? key ^ 0x80000000u : ~key; }
// the keys of the numbers span [SCORE_KEY_MIN, SCORE_KEY_MAX] = [key(-inf), key(+inf)]: what lies below is free for a caller's marks
constexpr uint32_t SCORE_KEY_MIN = 0x007fffffu, SCORE_KEY_MAX = 0xff800000u;

}  // namespace sslcr
