// Ranking metrics on the device (include/sslcr.h has the contracts and the definitions):
//   sort_pairs   a stable least-significant-digit radix sort of uint32 keys with uint32 values, B independent rows per call
//   rank_keys    float32 scores [n][C] -> order-preserving uint32 keys [C][n] and 0 / 1 / 2 class values [C][n], NaNs counted
//   auc_counts   the sorted rows -> (U2, P, N, nan) per column, U2 = sum over (positive, negative) pairs of 2 [s_i > s_j] + [s_i = s_j]
// Integer arithmetic only: there is no floating-point operation in this translation unit; a score is its bit pattern.  Every atomic
// is an integer add whose order does not reach the result, so two calls give equal bits.  Work proceeds between workgroups through
// launch boundaries only: no kernel waits for another workgroup, there is no look-back and no ticket, and every loop states its bound.
#include "kernels.hpp"
#include "map_common.hpp"
#include "score_key.hpp"

namespace sslcr {

constexpr int SORT_TILE = SSLCR_SORT_TILE, SORT_ITEMS = SORT_TILE / 256, SORT_RADIX = 256, SCAN_TRIP = SSLCR_RANK_SCAN_TRIP;
static_assert(SORT_TILE == 4096 && SORT_ITEMS == 16, "a wave owns 16 chunks of 64 consecutive keys; the AUC kernels pack 16 flags per thread");
static_assert(SCAN_TRIP == 64, "one trip of a partial scan is one wave");

// ------------------------------------------------------------------------------------------------ 1. radix sort
// One pass over the digit (key >> shift) & mask, three launches:
//   sort_hist     workgroup (tile, row): the tile's digit counts by LDS adds -> hist[row][digit][tile]
//   sort_scan     wave (digit, row): the exclusive sum of hist[row][digit][0 .. tiles) in place, SCAN_TRIP tiles a trip with a carry,
//                 and the digit's total -> tot[row][digit]
//   sort_scatter  workgroup (tile, row): the exclusive sum of tot[row] over the digits (256 values), the stable rank of every key
//                 within the tile, the tile reordered by digit in LDS, then stores that run along each digit's destination
// The rank within a tile: wave w owns keys [1024 w, 1024 w + 1024) of the tile as 16 chunks of 64 consecutive keys.  In a chunk the
// lanes holding one digit find each other with eight ballots (digit_peers); a key's rank among the wave's keys of its digit is the
// wave's count so far (wcnt[w][digit]) plus the peers in lower lanes, and the lowest peer adds the chunk's count.  Chunks, lanes and
// waves are all in key order, so equal digits keep their input order: the sort is stable.

// the lanes of this wave that are valid and hold the digit d; every lane must be active
__device__ __forceinline__ unsigned long long digit_peers(unsigned d, bool valid) {
  unsigned long long peers = __ballot(valid);
  for (int b = 0; b < 8; ++b) {                     // bound: 8 bits
    const bool bit = (d >> b) & 1u;
    const unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}

__global__ __launch_bounds__(256) void sort_hist_kernel(const uint32_t* keys, int* hist, int n, int tiles, int shift, unsigned mask) {
  __shared__ int h[SORT_RADIX];
  const int t = threadIdx.x, lane = t & 63, tile = blockIdx.x, row = blockIdx.y;
  h[t] = 0;
  __syncthreads();
  const uint32_t* k = keys + (int64_t)row * n;
  const int64_t base = (int64_t)tile * SORT_TILE;
  uint32_t key[SORT_ITEMS];
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {            // bound: 16 keys per thread, all loads in flight before the first add
    const int64_t i = base + j * 256 + t;
    key[j] = i < n ? k[i] : 0u;
  }
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const bool valid = base + j * 256 + t < n;
    const unsigned d = (key[j] >> shift) & mask;
    // a wave of one digit (a plateau of equal scores) adds once; otherwise every lane adds for itself: integer adds in any order
    if (__all(valid && d == (unsigned)__shfl((int)d, 0))) {
      if (lane == 0) atomicAdd(&h[d], 64);
    } else if (valid) {
      atomicAdd(&h[d], 1);
    }
  }
  __syncthreads();
  hist[((int64_t)row * SORT_RADIX + t) * tiles + tile] = h[t];
}

__global__ __launch_bounds__(256) void sort_scan_kernel(int* hist, int* tot, int tiles) {
  const int lane = threadIdx.x & 63, d = blockIdx.x * 4 + (threadIdx.x >> 6), row = blockIdx.y;
  int* h = hist + ((int64_t)row * SORT_RADIX + d) * tiles;
  int carry = 0;
  for (int base = 0; base < tiles; base += SCAN_TRIP) {                      // bound: ceil(tiles / SCAN_TRIP) trips
    const int i = base + lane;
    const int v = i < tiles ? h[i] : 0;
    const int incl = wave_incl_sum(v);
    if (i < tiles) h[i] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) tot[row * SORT_RADIX + d] = carry;
}

__global__ __launch_bounds__(256) void sort_scatter_kernel(const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout,
                                                           const int* hist, const int* tot, int n, int tiles, int shift, unsigned mask) {
  __shared__ uint32_t sk[SORT_TILE], sv[SORT_TILE];
  __shared__ int wcnt[4][SORT_RADIX], dstart[SORT_RADIX], gbase[SORT_RADIX], sh[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, tile = blockIdx.x, row = blockIdx.y;
  const int64_t rowoff = (int64_t)row * n, base = (int64_t)tile * SORT_TILE;
  const int count = (int)min((int64_t)SORT_TILE, (int64_t)n - base);
  for (int k = 0; k < 4; ++k) wcnt[k][t] = 0;
  __syncthreads();
  uint32_t key[SORT_ITEMS], val[SORT_ITEMS];
  int rank[SORT_ITEMS];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int c = 0; c < SORT_ITEMS; ++c) {            // bound: 16 chunks per wave; every load in flight before the first barrier below
    const int li = w * (SORT_TILE / 4) + c * 64 + lane;
    key[c] = li < count ? kin[rowoff + base + li] : 0u;
    val[c] = li < count ? vin[rowoff + base + li] : 0u;
  }
#pragma unroll
  for (int c = 0; c < SORT_ITEMS; ++c) {
    const bool valid = w * (SORT_TILE / 4) + c * 64 + lane < count;
    const unsigned d = (key[c] >> shift) & mask;
    const unsigned long long peers = digit_peers(d, valid);
    const int before = wcnt[w][d];
    rank[c] = before + __popcll(peers & below);
    __syncthreads();                                // every read of the wave's counts before the chunk's adds
    if (valid && __ffsll(peers) - 1 == lane) wcnt[w][d] = before + __popcll(peers);
    __syncthreads();
  }
  // thread t = digit t: the tile's count, its start within the tile, each wave's start within the digit, the destination of its first key
  const int c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t], c3 = wcnt[3][t];
  int total;
  const int ds = block_excl_sum(c0 + c1 + c2 + c3, sh, &total);
  const int dg = block_excl_sum(tot[row * SORT_RADIX + t], sh, &total);      // the keys of the row with a smaller digit
  wcnt[0][t] = ds;
  wcnt[1][t] = ds + c0;
  wcnt[2][t] = ds + c0 + c1;
  wcnt[3][t] = ds + c0 + c1 + c2;
  dstart[t] = ds;
  gbase[t] = dg + hist[((int64_t)row * SORT_RADIX + t) * tiles + tile];       // ... plus those with this digit in the tiles before
  __syncthreads();
#pragma unroll
  for (int c = 0; c < SORT_ITEMS; ++c) {
    const int li = w * (SORT_TILE / 4) + c * 64 + lane;
    const unsigned d = (key[c] >> shift) & mask;
    const int pos = wcnt[w][d] + rank[c];
    if (li < count && (unsigned)pos < (unsigned)SORT_TILE) {
      sk[pos] = key[c];
      sv[pos] = val[c];
    }
  }
  __syncthreads();
  for (int j = 0; j < SORT_ITEMS; ++j) {            // bound: 16 slots per thread; consecutive threads store consecutive dwords of a digit
    const int p = j * 256 + t;
    if (p < count) {
      const uint32_t k = sk[p];
      const unsigned d = (k >> shift) & mask;
      const int g = gbase[d] + (p - dstart[d]);
      if ((unsigned)g < (unsigned)n) {              // holds whenever the three launches saw the same keys
        kout[rowoff + g] = k;
        vout[rowoff + g] = sv[p];
      }
    }
  }
}

hipError_t launch_sort_pairs(const sslcr_sort_desc& a, hipStream_t st) {
  const int tiles = (int)(((int64_t)a.n + SORT_TILE - 1) / SORT_TILE);
  int* hist = static_cast<int*>(a.workspace);
  int* tot = hist + (int64_t)a.B * SORT_RADIX * tiles;
  int src = 0;
  for (int shift = a.lo; shift < a.hi; shift += 8) {                         // bound: ceil((hi - lo) / 8) <= 4 passes
    const int bits = a.hi - shift < 8 ? a.hi - shift : 8;
    const unsigned mask = (1u << bits) - 1u;
    hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)tiles, (unsigned)a.B), dim3(256), 0, st, a.keys[src], hist, a.n, tiles, shift, mask);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(SORT_RADIX / 4, (unsigned)a.B), dim3(256), 0, st, hist, tot, tiles);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)tiles, (unsigned)a.B), dim3(256), 0, st, a.keys[src], a.values[src],
                       a.keys[src ^ 1], a.values[src ^ 1], hist, tot, a.n, tiles, shift, mask);
    src ^= 1;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. keys and class values
__global__ __launch_bounds__(256) void rank_keys_kernel(const sslcr_rank_keys_desc a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < a.n;
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(a.scores);
  const bool ok = in && (!a.valid || a.valid[i] != 0);
  const int64_t target = in ? a.target[i] : 0;
  unsigned long long* nan = reinterpret_cast<unsigned long long*>(a.nan);
  for (int c = 0; c < a.C; ++c) {                   // bound: C columns
    uint32_t b = in ? bits[i * a.C + c] : 0u;
    const bool is_nan = ok && score_is_nan(b);
    const uint32_t key = score_key(b);              // score_key.hpp: -0 ties with +0
    const int64_t positive = a.positive ? a.positive[c] : (int64_t)c;
    const uint32_t value = (!ok || is_nan) ? 2u : (target == positive ? 1u : 0u);
    if (in) {
      a.keys[(int64_t)c * a.n + i] = key;
      a.values[(int64_t)c * a.n + i] = value;
    }
    wave_vote_add(nan + c, is_nan);
  }
}

hipError_t launch_rank_keys(const sslcr_rank_keys_desc& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.nan, 0, (size_t)a.C * sizeof(int64_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rank_keys_kernel, dim3((unsigned)(((int64_t)a.n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 3. the pair counts of a sorted row
// Ascending keys.  A RUN is a maximal stretch of equal keys; its head is its first element, its tail its last.  For a positive i,
//   A(i) = the negatives before the head of i's run  (those with a smaller score),
//   Z(i) = the negatives after the tail of i's run   (those with a larger score),
// and its pairs count 2 A(i) + (N - A(i) - Z(i)) = A(i) + N - Z(i), so U2 = sum over the positives of A + N - Z.  The exclusive count e of
// negatives before an element does not decrease along the row, so A(i) = the max of e over the heads at or before i; Z mirrors it
// from the other end with the tails.  An element with value 2 is neither: it may sit anywhere in a run.
//   auc_partials  workgroup (block of SORT_TILE elements, column): negatives, positives, e at the block's last head, and the
//                 negatives after the block's first tail, both counted within the block (-1: no head / no tail)
//   auc_scan      one wave per column: the blocks before / after each block summed and max-ed, SCAN_TRIP blocks a trip with carries,
//                 in block order: (negatives before, A carried in, negatives after, Z carried in); and P, N, nan into the result
//   auc_apply     workgroup (block, column): A and Z of every positive from the carries; one integer add of the block's sum
struct AucThread {
  unsigned heads, tails, neg, pos;                  // bit j: element j of the thread's 16
};

__device__ __forceinline__ AucThread auc_load(const uint32_t* k, const uint32_t* v, int64_t i0, int n) {
  AucThread r = {0u, 0u, 0u, 0u};
  uint32_t prev = (i0 > 0 && i0 - 1 < n) ? k[i0 - 1] : 0u;
  uint32_t cur = i0 < n ? k[i0] : 0u;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {            // bound: 16 elements per thread
    const int64_t i = i0 + j;
    const uint32_t next = i + 1 < n ? k[i + 1] : 0u;
    if (i < n) {
      const uint32_t value = v[i];
      if (i == 0 || prev != cur) r.heads |= 1u << j;
      if (i == (int64_t)n - 1 || next != cur) r.tails |= 1u << j;
      if (value == 0u) r.neg |= 1u << j;
      if (value == 1u) r.pos |= 1u << j;
    }
    prev = cur;
    cur = next;
  }
  return r;
}
// the thread's negatives before its last head / after its first tail (-1: it has none)
__device__ __forceinline__ int auc_head_pre(const AucThread& r) {
  if (!r.heads) return -1;
  const int j = 31 - __clz((int)r.heads);
  return __popc(r.neg & ((1u << j) - 1u));
}
__device__ __forceinline__ int auc_tail_post(const AucThread& r) {
  if (!r.tails) return -1;
  const int j = __ffs((int)r.tails) - 1;
  return __popc(r.neg >> (j + 1));
}

// work: per (column, block) 8 ints: 0 negatives, 1 positives, 2 e at the last head, 3 negatives after the first tail (block-local),
// 4 negatives before the block, 5 A carried in, 6 negatives after the block, 7 Z carried in (row-global; -1 = none)
__global__ __launch_bounds__(256) void auc_partials_kernel(const sslcr_auc_desc a, int nb) {
  __shared__ int sh[4];
  const int t = threadIdx.x, blk = blockIdx.x, c = blockIdx.y;
  const int64_t rowoff = (int64_t)c * a.n;
  const AucThread r = auc_load(a.keys + rowoff, a.values + rowoff, (int64_t)blk * SORT_TILE + t * SORT_ITEMS, a.n);
  const int neg = __popc(r.neg);
  int negs, poss, head_e, tail_s;
  const int ex = block_excl_sum(neg, sh, &negs);
  block_excl_sum(__popc(r.pos), sh, &poss);
  const int hp = auc_head_pre(r), tp = auc_tail_post(r);
  block_scan_max(hp < 0 ? -1 : ex + hp, false, -1, sh, &head_e);
  block_scan_max(tp < 0 ? -1 : negs - ex - neg + tp, true, -1, sh, &tail_s);
  if (t == 0) {
    int* p = a.work + ((int64_t)c * nb + blk) * 8;
    p[0] = negs;
    p[1] = poss;
    p[2] = head_e;
    p[3] = tail_s;
  }
}

__global__ __launch_bounds__(64) void auc_scan_kernel(const sslcr_auc_desc a, int nb) {
  const int lane = threadIdx.x, c = blockIdx.x;
  int* w = a.work + (int64_t)c * nb * 8;
  int carry = 0, carry_m = -1;
  long long pos = 0;
  for (int base = 0; base < nb; base += SCAN_TRIP) {                         // bound: ceil(nb / SCAN_TRIP) trips, first block first
    const int b = base + lane;
    const int neg = b < nb ? w[(int64_t)b * 8] : 0, he = b < nb ? w[(int64_t)b * 8 + 2] : -1;
    pos += b < nb ? w[(int64_t)b * 8 + 1] : 0;
    const int incl = wave_incl_sum(neg), ex = carry + incl - neg;
    const int im = wave_incl_max(he < 0 ? -1 : ex + he);
    int em = __shfl_up(im, 1);
    if (lane == 0) em = -1;
    if (b < nb) {
      w[(int64_t)b * 8 + 4] = ex;
      w[(int64_t)b * 8 + 5] = max(em, carry_m);
    }
    carry += __shfl(incl, 63);
    carry_m = max(carry_m, __shfl(im, 63));
  }
  const int negatives = carry;
  carry = 0, carry_m = -1;
  for (int base = 0; base < nb; base += SCAN_TRIP) {                         // bound: the same trips, last block first
    const int b = nb - 1 - (base + lane);
    const int neg = b >= 0 ? w[(int64_t)b * 8] : 0, ts = b >= 0 ? w[(int64_t)b * 8 + 3] : -1;
    const int incl = wave_incl_sum(neg), ex = carry + incl - neg;
    const int im = wave_incl_max(ts < 0 ? -1 : ex + ts);
    int em = __shfl_up(im, 1);
    if (lane == 0) em = -1;
    if (b >= 0) {
      w[(int64_t)b * 8 + 6] = ex;
      w[(int64_t)b * 8 + 7] = max(em, carry_m);
    }
    carry += __shfl(incl, 63);
    carry_m = max(carry_m, __shfl(im, 63));
  }
  pos = (long long)wave_sum((unsigned long long)pos);
  if (lane == 0) {
    a.counts[c * 4 + 0] = 0;
    a.counts[c * 4 + 1] = pos;
    a.counts[c * 4 + 2] = negatives;
    a.counts[c * 4 + 3] = a.nan ? a.nan[c] : 0;
  }
}

__global__ __launch_bounds__(256) void auc_apply_kernel(const sslcr_auc_desc a, int nb) {
  __shared__ int sh[4];
  __shared__ unsigned long long acc[4];
  const int t = threadIdx.x, lane = t & 63, blk = blockIdx.x, c = blockIdx.y;
  const int64_t rowoff = (int64_t)c * a.n;
  const AucThread r = auc_load(a.keys + rowoff, a.values + rowoff, (int64_t)blk * SORT_TILE + t * SORT_ITEMS, a.n);
  const int* p = a.work + ((int64_t)c * nb + blk) * 8;
  const int before = p[4], a_in = p[5], after = p[6], z_in = p[7];
  const unsigned long long negatives = (unsigned long long)a.counts[c * 4 + 2];
  const int neg = __popc(r.neg);
  int negs, unused;
  const int ex = block_excl_sum(neg, sh, &negs);
  const int hp = auc_head_pre(r), tp = auc_tail_post(r);
  int e = before + ex, z = after + negs - ex - neg;  // the negatives before the thread's first element / after its last
  int cur_a = max(a_in, block_scan_max(hp < 0 ? -1 : e + hp, false, -1, sh, &unused));
  int cur_z = max(z_in, block_scan_max(tp < 0 ? -1 : z + tp, true, -1, sh, &unused));
  unsigned long long sum = 0;                       // over the thread's positives: A + N - Z, each term >= 0
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    if ((r.heads >> j) & 1u) cur_a = e;
    if ((r.pos >> j) & 1u) sum += (unsigned long long)cur_a + negatives;
    if ((r.neg >> j) & 1u) ++e;
  }
#pragma unroll
  for (int j = SORT_ITEMS - 1; j >= 0; --j) {
    if ((r.tails >> j) & 1u) cur_z = z;
    if ((r.pos >> j) & 1u) sum -= (unsigned long long)cur_z;
    if ((r.neg >> j) & 1u) ++z;
  }
  sum = wave_sum(sum);
  if (lane == 0) acc[t >> 6] = sum;
  __syncthreads();
  if (t == 0) {
    const unsigned long long all = acc[0] + acc[1] + acc[2] + acc[3];
    if (all) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + c * 4, all);
  }
}

hipError_t launch_auc_counts(const sslcr_auc_desc& a, hipStream_t st) {
  const int nb = (int)(((int64_t)a.n + SORT_TILE - 1) / SORT_TILE);
  hipLaunchKernelGGL(auc_partials_kernel, dim3((unsigned)nb, (unsigned)a.C), dim3(256), 0, st, a, nb);
  hipLaunchKernelGGL(auc_scan_kernel, dim3((unsigned)a.C), dim3(64), 0, st, a, nb);
  hipLaunchKernelGGL(auc_apply_kernel, dim3((unsigned)nb, (unsigned)a.C), dim3(256), 0, st, a, nb);
  return hipGetLastError();
}

}  // namespace sslcr
