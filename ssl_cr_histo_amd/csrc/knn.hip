// k-nearest-neighbour feature probe (include/sslcr.h has the contracts and the definitions):
//   knn_topk      the k bank rows with the greatest fp32 dot product per query; the nq x nb similarities never reach HBM
//   knn_merge     the S per-slice lists of a query merged, decoded into scores and indices
//   l2_normalize  x / max(||x||, eps) per row, the norm in float64 (cosine similarity = the dot product of normalised rows)
//   knn_vote      uniform / softmax-weighted class votes or the mean target of the neighbours, and the confusion counts
// The similarity is exact fp32 on v_mfma_f32_16x16x4_f32: an fmaf chain over d in rising order from +0, so its bits do not depend on
// the tile, the slice count or the route.  The selection compares 64-bit integer keys (score_key.hpp's key, then the lower bank index),
// a total order, so neither do the neighbours.  Work passes between workgroups at the launch boundary only: no kernel waits for another
// workgroup, there is no look-back, no ticket and no floating-point atomic, and every loop states its bound.
#include "kernels.hpp"
#include "score_key.hpp"
#include "softmax_row.hpp"

namespace sslcr {

constexpr int KT = SSLCR_KNN_TILE, KC = SSLCR_KNN_CHUNK;
constexpr int KNN_PITCH = KC + 4;                   // floats per LDS operand row: the 16 rows of a fragment read hit 64 different banks
constexpr int KNN_SPITCH = KT + 4;                  // floats per LDS score row: 4 rows on = 16 banks on, so the accumulator stores of the lane
                                                    // groups g = 0, 1 (rows 4 g + r, columns li) fall on 32 different banks
static_assert(KT == 64 && KC == 64, "a wave's lanes are the 64 candidates of a bank tile; a thread stages 4 x 16 bytes per operand and chunk");
static_assert(SSLCR_KNN_MAX_K == 64, "one list slot per lane");
constexpr int KNN_SLOTS = 512;                      // workgroups of knn_topk_kernel the chip holds at once: two a CU (LDS), 256 CUs
static_assert(2 * KT * KNN_PITCH >= KT * KNN_SPITCH, "the score tile lies in the operand buffer");

typedef unsigned long long knn_key_t;

// ------------------------------------------------------------------------------------------------ keys
// (score key << 32) | ~index: greater = better.  0 = the empty slot; NaN scores share the score key 1, below every number's.
constexpr uint32_t KNN_NAN_KEY = 1u;
static_assert(KNN_NAN_KEY < SCORE_KEY_MIN, "a NaN ranks below -inf and above the empty slot");
__device__ __forceinline__ knn_key_t knn_key(float s, uint32_t j) {
  const uint32_t b = __float_as_uint(s);
  const uint32_t hi = score_is_nan(b) ? KNN_NAN_KEY : score_key(b);
  return ((knn_key_t)hi << 32) | (knn_key_t)(~j);
}
__device__ __forceinline__ void knn_decode(knn_key_t key, float* score, int32_t* index) {
  const uint32_t hi = (uint32_t)(key >> 32);
  if (key == 0ull) { *score = __uint_as_float(0xff800000u); *index = -1; return; }
  *index = (int32_t)(~(uint32_t)key);
  *score = __uint_as_float(hi == KNN_NAN_KEY ? 0x7fc00000u : score_from_key(hi));
}
__device__ __forceinline__ knn_key_t shfl_xor_key(knn_key_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return ((knn_key_t)hi << 32) | lo;
}
__device__ __forceinline__ knn_key_t shfl_key(knn_key_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((knn_key_t)hi << 32) | lo;
}

// The sort-and-merge over the 64 lanes of a wave.  list: the query's best 64 keys so far, DESCENDING by lane (empty slots 0 at the
// end); cand: one candidate per lane in any order (0 = none).  Returns the best 64 of the 128, descending by lane.  The candidates are
// sorted ASCENDING (bitonic sort, 21 compare-exchanges); max(list[l], cand[l]) then holds the best 64 of the union as a bitonic
// sequence, which 6 more exchanges sort.  Keys are distinct (a bank row occurs once per query) except for the 0s, whose order is
// immaterial.  Every lane must be active.
__device__ __forceinline__ knn_key_t sort_ascending(knn_key_t cand, int lane) {
  for (int size = 2; size <= 64; size <<= 1) {      // bound: 6 sizes ...
    for (int j = size >> 1; j > 0; j >>= 1) {       // ... of at most 6 exchanges
      const knn_key_t other = shfl_xor_key(cand, j);
      const bool up = (lane & size) == 0, lower = (lane & j) == 0;
      const knn_key_t lo = cand < other ? cand : other, hi = cand < other ? other : cand;
      cand = (lower == up) ? lo : hi;
    }
  }
  return cand;
}
// list descending, asc ASCENDING by lane -> the best 64 of both, descending
__device__ __forceinline__ knn_key_t merge_sorted(knn_key_t list, knn_key_t asc, int lane) {
  knn_key_t v = list > asc ? list : asc;
  for (int j = 32; j > 0; j >>= 1) {                // bound: 6 exchanges
    const knn_key_t other = shfl_xor_key(v, j);
    const bool lower = (lane & j) == 0;
    const knn_key_t lo = v < other ? v : other, hi = v < other ? other : v;
    v = lower ? hi : lo;
  }
  return v;
}
__device__ __forceinline__ knn_key_t topk_merge(knn_key_t list, knn_key_t cand, int lane) { return merge_sorted(list, sort_ascending(cand, lane), lane); }

// ------------------------------------------------------------------------------------------------ 1. fused similarity and top-k
// Workgroup (query tile, slice): 64 queries against the slice's bank tiles of 64 rows.  Per bank tile the 64 x 64 similarities are
// accumulated over D in chunks of 64: both operand tiles are fetched with whole 256-byte rows per 16 lanes (a lane fetching its own
// row's 16 bytes has the coalescer serialise 64 segments: heads.hip's gemm_f32_lds_kernel has the measurement), the next chunk's
// fetch in flight during this chunk's MFMAs, and staged into LDS with the 4 x 4 transpose of every 16 elements that makes the
// fragment reads deliver RISING d: position 16 u + 4 g + e of a row holds element d = 16 u + 4 e + g, so the 16-byte read of lane
// (li, g) at 16 u + 4 g feeds MFMA e with d = 16 u + 4 e + g -- MFMA e of group u covers d = 16 u + 4 e .. + 3, lane group g being
// the k index of v_mfma_f32_16x16x4_f32.  Wave (wm, wn) owns 32 queries x 32 bank rows as 2 x 2 accumulator tiles: four independent
// accumulators against the 40-cycle dependent latency.  The finished scores go through LDS (in the operand buffer) to the selection:
// wave w owns queries 16 w .. 16 w + 15, lane l is bank row l of the tile.
__global__ __launch_bounds__(256) void knn_topk_kernel(const sslcr_knn_desc a, int tiles_per_slice, int bank_tiles) {
  __shared__ __attribute__((aligned(16))) float ops[2][KT * KNN_PITCH];      // [0] queries, [1] bank rows; then the score tile
  __shared__ knn_key_t lists[KT][64];               // per query: its best 64 keys so far, descending
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int D = a.D;
  const int64_t q0 = (int64_t)blockIdx.x * KT;
  const int slice = blockIdx.y;
  const int t_lo = slice * tiles_per_slice, t_hi = min(bank_tiles, t_lo + tiles_per_slice);
  float* sc = &ops[0][0];

  for (int i = tid; i < KT * 64; i += 256) (&lists[0][0])[i] = 0ull;         // bound: 16 per thread
  __syncthreads();                                  // a wave reads (and, for an empty slice, stores) list rows that other waves zeroed
  knn_key_t thr = 0ull;                             // lane q < 16 of wave w: the current k-th key of query 16 w + q

  // a thread's four 16-byte pieces per operand and chunk: piece c = tid + 256 p is row c >> 4, elements 4 (c & 15) .. + 3
  f32x4_t ra[4], rb[4];
  auto fetch = [&](int64_t b0, int kb) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c = tid + 256 * p, row = c >> 4, d = kb + 4 * (c & 15);
      const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
      const bool din = d < D;                       // D % 4 == 0: a piece lies inside D or outside it
      ra[p] = (din && q0 + row < a.nq) ? *reinterpret_cast<const f32x4_t*>(a.queries + (q0 + row) * D + d) : zero;
      rb[p] = (din && b0 + row < a.nb) ? *reinterpret_cast<const f32x4_t*>(a.bank + (b0 + row) * D + d) : zero;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c = tid + 256 * p, row = c >> 4, u = (c & 15) >> 2, s = c & 3;
      float* pa = &ops[0][row * KNN_PITCH + 16 * u + s];
      float* pb = &ops[1][row * KNN_PITCH + 16 * u + s];
#pragma unroll
      for (int e = 0; e < 4; ++e) { pa[4 * e] = ra[p][e]; pb[4 * e] = rb[p][e]; }
    }
  };

  for (int t = t_lo; t < t_hi; ++t) {               // bound: tiles_per_slice bank tiles
    const int64_t b0 = (int64_t)t * KT;
    f32x4_t acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    fetch(b0, 0);
    for (int kb = 0; kb < D; kb += KC) {            // bound: ceil(D / 64) chunks, rising d
      __syncthreads();                              // the readers of the buffer are done: the chunk before, or the selection of the tile before
      stage();
      __syncthreads();
      if (kb + KC < D) fetch(b0, kb + KC);
      const float* la = &ops[0][(32 * wm + li) * KNN_PITCH + 4 * g];
      const float* lb = &ops[1][(32 * wn + li) * KNN_PITCH + 4 * g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f32x4_t fa[2], fb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          fa[m] = *reinterpret_cast<const f32x4_t*>(la + 16 * m * KNN_PITCH + 16 * u);
          fb[m] = *reinterpret_cast<const f32x4_t*>(lb + 16 * m * KNN_PITCH + 16 * u);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[mi][e], fb[ni][e], acc[mi][ni], 0, 0, 0);
      }
    }
    __syncthreads();                                // every fragment read of the last chunk before the scores overwrite the operands
    // D[row = 4 g + r][col = li] of tile (mi, ni): query 32 wm + 16 mi + 4 g + r, bank row 32 wn + 16 ni + li
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[(32 * wm + 16 * mi + 4 * g + r) * KNN_SPITCH + 32 * wn + 16 * ni + li] = acc[mi][ni][r];
    __syncthreads();
    // selection: the tile's candidates of each of the wave's 16 queries against the query's k-th key; most tiles insert nothing
    const int64_t j = b0 + lane;
    auto candidate = [&](int q) -> knn_key_t {
      const int row = 16 * wave + q;
      const int64_t qi = q0 + row;
      const bool ok = qi < a.nq && j < a.nb_valid && !(a.self_offset >= 0 && j == qi + a.self_offset);
      return ok ? knn_key(sc[row * KNN_SPITCH + lane], (uint32_t)j) : 0ull;
    };
    // first all 16 tests (unrolled: the score reads are in flight together, the k-th keys come by v_readlane), then the rare merges
    unsigned pass = 0u;                             // wave-uniform: bit q = some candidate of query q beats its k-th key
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const knn_key_t kth = ((knn_key_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(thr >> 32), q) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)thr, q);
      if (__ballot(candidate(q) > kth) != 0ull) pass |= 1u << q;
    }
    while (pass) {                                  // bound: 16 queries per wave
      const int q = __ffs((int)pass) - 1;
      pass &= pass - 1u;
      const int row = 16 * wave + q;
      const knn_key_t merged = topk_merge(lists[row][lane], candidate(q), lane);
      lists[row][lane] = merged;
      const knn_key_t now = shfl_key(merged, a.k - 1);
      if (lane == q) thr = now;
    }
  }
  // the partial lists: k keys per query of this (tile, slice); a wave stores its own queries' lists (no barrier: it wrote them itself)
  knn_key_t* ws = static_cast<knn_key_t*>(a.workspace);
  for (int q = 0; q < 16; ++q) {                    // bound: 16 queries per wave
    const int row = 16 * wave + q;
    const int64_t qi = q0 + row;
    if (qi < a.nq && lane < a.k) ws[((int64_t)slice * a.nq + qi) * a.k + lane] = lists[row][lane];
  }
}

// one wave per query: the S lists of k keys (each descending) merged with the same sort-and-merge, then decoded
__global__ __launch_bounds__(256) void knn_merge_kernel(const sslcr_knn_desc a, int S) {
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= a.nq) return;                           // wave-uniform
  const knn_key_t* ws = static_cast<const knn_key_t*>(a.workspace);
  knn_key_t list = 0ull;
  const int p = 63 - lane;                          // a slice's list is descending: read backwards it is ascending by lane, no sort needed
  for (int s = 0; s < S; ++s) {                     // bound: S slices
    const knn_key_t asc = p < a.k ? ws[((int64_t)s * a.nq + qi) * a.k + p] : 0ull;
    list = merge_sorted(list, asc, lane);
  }
  if (lane < a.k) {
    float score;
    int32_t index;
    knn_decode(list, &score, &index);
    a.scores[qi * a.k + lane] = score;
    a.indices[qi * a.k + lane] = index;
  }
}

const char* knn_plan(int nq, int nb, int D, int k, int slices_hint, KnnPlan* out) {
  if (nq < 0) return "nq < 0";
  if (nb < 1 || nb >= 0x7fffffff - KT) return "nb outside [1, 2^31 - 64)";
  if (D < 4 || D > SSLCR_KNN_MAX_D || D % 4 != 0) return "D % 4 == 0 and 4 <= D <= 2048";
  if (k < 1 || k > SSLCR_KNN_MAX_K) return "k outside [1, 64]";
  if (slices_hint < 0) return "slices < 0";
  const int q_tiles = nq == 0 ? 0 : (int)(((int64_t)nq + KT - 1) / KT), b_tiles = (int)(((int64_t)nb + KT - 1) / KT);
  int S = 1;
  if (slices_hint > 0) {
    S = slices_hint;                                // (under a hint a trailing slice may be empty: it writes empty lists)
    if (S > SSLCR_KNN_MAX_SLICES) S = SSLCR_KNN_MAX_SLICES;
    if (S > b_tiles) S = b_tiles;
  } else if (q_tiles > 0) {
    // The chip runs KNN_SLOTS workgroups at a time (two a CU, 256 CUs), in rounds: q_tiles * S workgroups fill
    // q_tiles * S / (rounds * KNN_SLOTS) of them.  The smallest S that fills 95 %, else the S that fills most; at least 4 bank tiles
    // a slice (a slice's list costs every query a merge trip), no empty slice.  (Measured on the 7 180 x 100 000 case: S = 5, 565
    // workgroups = 1.1 rounds, ran 22.4 ms where one slice ran 38.6 ms: the second round's 53 workgroups had the chip to themselves.)
    int smax = b_tiles / 4;
    if (smax > SSLCR_KNN_MAX_SLICES) smax = SSLCR_KNN_MAX_SLICES;
    double best = 0.0;
    for (int s = 1; s <= smax; ++s) {               // bound: at most SSLCR_KNN_MAX_SLICES candidates
      const int t = (b_tiles + s - 1) / s;
      if ((b_tiles + t - 1) / t != s) continue;     // this s would leave a slice empty
      const int64_t wgs = (int64_t)q_tiles * s, rounds = (wgs + KNN_SLOTS - 1) / KNN_SLOTS;
      const double fill = (double)wgs / (double)(rounds * KNN_SLOTS);
      if (fill > best + 1e-9) { best = fill; S = s; }
      if (fill >= 0.95) break;
    }
  }
  if (S < 1) S = 1;
  if ((int64_t)q_tiles * S > 0x7fffffff) return "nq / 64 * slices >= 2^31";
  const int tps = (b_tiles + S - 1) / S;
  out->form = S > 1 ? SSLCR_KNN_SLICED : SSLCR_KNN_DIRECT;
  out->tile_q = KT; out->tile_b = KT; out->chunk = KC;
  out->slices = S;
  out->tiles_per_slice = tps;
  out->grid[0] = q_tiles * S;
  out->grid[1] = (int)(((int64_t)nq + 3) / 4);
  out->lds_bytes = sizeof(float) * 2 * KT * KNN_PITCH + sizeof(knn_key_t) * KT * 64;
  out->workspace_bytes = (size_t)S * (size_t)nq * (size_t)k * sizeof(knn_key_t);
  return nullptr;
}

hipError_t launch_knn_topk(const sslcr_knn_desc& a, const KnnPlan& p, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  // the bank tiles that hold an admissible row: those past nb_valid are not walked (their slices write empty lists)
  const int q_tiles = p.grid[0] / p.slices, b_tiles = (int)(((int64_t)(a.nb_valid < a.nb ? a.nb_valid : a.nb) + KT - 1) / KT);
  hipLaunchKernelGGL(knn_topk_kernel, dim3((unsigned)q_tiles, (unsigned)p.slices), dim3(256), 0, st, a, p.tiles_per_slice, b_tiles);
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)p.grid[1]), dim3(256), 0, st, a, p.slices);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. row normalisation
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* x, float* y, int n, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                             // wave-uniform
  const float* xr = x + row * D;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {              // bound: ceil(D / 64) elements per lane, rising d
    const double v = (double)xr[d];
    s += v * v;
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);                   // bound: 6 steps of a butterfly: a fixed order, every lane ends with the total
  const float norm = (float)sqrt(s);
  const float den = fmaxf(norm, eps);
  float* yr = y + row * D;
  for (int d = lane; d < D; d += 64) yr[d] = __fdiv_rn(xr[d], den);          // bound: as above
}

hipError_t launch_l2_normalize(const float* x, float* y, int n, int D, float eps, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, st, x, y, n, D, eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 3. votes
// one thread per query; a query's votes accumulate in its own row of the output (this thread alone reads and writes it)
__global__ __launch_bounds__(256) void knn_vote_kernel(const sslcr_knn_vote_desc a) {
  __shared__ unsigned cells[CONFUSION_MAX_C * CONFUSION_MAX_C];
  const bool regress = a.mode == SSLCR_KNN_VOTE_REGRESS;
  const int C = a.C, k = a.k;
  if (a.confusion) confusion_clear(cells, C * C);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.nq) {
    const int32_t* idx = a.indices + i * k;
    if (regress) {
      float sum = 0.f;
      int count = 0;
      for (int r = 0; r < k; ++r) {                 // bound: k neighbours, in rank order
        const int32_t j = idx[r];
        if (j < 0 || j >= a.nb) continue;
        sum += a.targets[j];
        ++count;
      }
      a.pred_value[i] = __fdiv_rn(sum, (float)count);
    } else {
      float* v = a.votes + i * C;
      for (int c = 0; c < C; ++c) v[c] = 0.f;       // bound: C classes
      const float s0 = a.mode == SSLCR_KNN_VOTE_SOFTMAX ? a.scores[i * k] : 0.f;
      for (int r = 0; r < k; ++r) {                 // bound: k neighbours, in rank order
        const int32_t j = idx[r];
        if (j < 0 || j >= a.nb) continue;
        const int64_t c = a.labels[j];
        if (c < 0 || c >= C) continue;
        const float w = a.mode == SSLCR_KNN_VOTE_SOFTMAX ? expf(__fdiv_rn(a.scores[i * k + r] - s0, a.temperature)) : 1.f;
        v[c] += w;
      }
      int best = 0;
      float m = v[0];
      for (int c = 1; c < C; ++c)                   // the most votes; a tie goes to the lowest class
        if (v[c] > m) { m = v[c]; best = c; }
      a.pred[i] = best;
      if (a.confusion) confusion_count(cells, C, a.query_labels[i], best);
    }
  }
  if (a.confusion) confusion_flush(cells, C * C, a.confusion);
}

hipError_t launch_knn_vote(const sslcr_knn_vote_desc& a, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)(((int64_t)a.nq + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sslcr
