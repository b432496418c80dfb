// t-SNE embedding (include/sslcr.h has the contracts; tests/_tsne_ref.py is the float64 restatement, pinned to sklearn 1.7.2):
//   tsne_pair_dist2   squared Euclidean distances to the neighbours knn_topk found, summed in float64 in rising d
//   tsne_affinities   sklearn's _binary_search_perplexity, one wave per row, one neighbour per lane
//   tsne_repulsion    the EXACT O(n^2) repulsive sum, per (row, column slice) fp32 partials; tsne_zfold folds sum q into the float64 Z
//   tsne_update       folds the partials, walks the row's CSR entries, forms the gradient, applies gains and momentum
//   tsne_kl           KL and |grad| into one row of a device log
// Work passes between workgroups at the launch boundary only: no floating-point atomics, no tickets, no spins; every loop states
// its bound, every reduction is a fixed tree, so two calls return equal bits.
#include <float.h>

#include "kernels.hpp"

namespace sslcr {

constexpr int TT = SSLCR_TSNE_TILE, TC = SSLCR_TSNE_CHUNK;
constexpr int TSNE_FILL = 1024;                     // workgroups that fill the chip: four a CU, 256 CUs
constexpr int TSNE_FOLD = 1024;                     // threads of the one-workgroup folds
static_assert(TC % TT == 0, "a workgroup stages a chunk in whole trips");

// xor-butterfly over the 64 lanes: a fixed tree (a + b is commutative, so both partners of a step hold the same bits)
__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);                   // bound: 6 steps
  return v;
}

// the tree of a one-workgroup fold: TSNE_FOLD values in LDS, halved 10 times
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();                                  // the fold before has been read
  sh[tid] = v;
  __syncthreads();
  for (int h = TSNE_FOLD / 2; h >= 1; h >>= 1) {    // bound: 10 halvings
    if (tid < h) sh[tid] += sh[tid + h];
    __syncthreads();
  }
  return sh[0];
}

// ------------------------------------------------------------------------------------------------ 1. neighbour distances
__global__ __launch_bounds__(256) void tsne_pair_dist2_kernel(const float* x, const int32_t* indices, float* dist2, int n, int D, int k) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n || lane >= k) return;
  const int32_t j = indices[i * k + lane];
  float out = __uint_as_float(0x7f800000u);
  if (j >= 0 && j < n) {
    const float* xi = x + i * D;
    const float* xj = x + (int64_t)j * D;
    double s = 0.0;
#pragma unroll 4
    for (int d = 0; d < D; ++d) {                   // bound: D elements, rising d
      const double t = (double)xi[d] - (double)xj[d];                        // exact
      s = __dadd_rn(s, __dmul_rn(t, t));            // two roundings: no contraction
    }
    out = (float)s;
  }
  dist2[i * k + lane] = out;
}

hipError_t launch_tsne_pair_dist2(const float* x, const int32_t* indices, float* dist2, int n, int D, int k, hipStream_t st) {
  hipLaunchKernelGGL(tsne_pair_dist2_kernel, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, st, x, indices, dist2, n, D, k);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. conditional affinities
__global__ __launch_bounds__(256) void tsne_affinities_kernel(const float* dist2, float* P, double* beta_out, int n, int k, double desired) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                               // wave-uniform
  const bool in = lane < k;
  const double d = in ? (double)dist2[i * k + lane] : 0.0;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, p = 0.0;
  for (int step = 0; step < 100; ++step) {          // bound: sklearn's n_steps; every test below is wave-uniform
    const double e = in ? exp(-d * beta) : 0.0;
    double s = wave_sum(e);
    if (s == 0.0) s = 1e-8;
    p = e / s;
    const double sdp = wave_sum(d * p);
    const double diff = log(s) + beta * sdp - desired;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  if (in) P[i * k + lane] = (float)p;
  if (lane == 0) beta_out[i] = beta;
}

hipError_t launch_tsne_affinities(const float* dist2, float* P, double* beta, int n, int k, float perplexity, hipStream_t st) {
  hipLaunchKernelGGL(tsne_affinities_kernel, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, st, dist2, P, beta, n, k,
                     log((double)perplexity));
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 3. repulsion
// Workgroup (row tile, slice): thread t owns row tile * TT + t and walks the slice's columns in chunks of TC points staged in LDS;
// every lane reads the same LDS address (a broadcast).  Per pair: 2 subtractions, d2 = fma(dy, dy, dx * dx), 1 + d2, v_rcp_f32
// (1 ulp), q * q, and the three accumulations (one add, two fmas), in rising j.
__global__ __launch_bounds__(TT) void tsne_repulsion_kernel(const float2* y, float4* ws, int n, int S, int chunks, int cps) {
  __shared__ float2 pts[TC];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * TT + tid, slice = blockIdx.y;
  const bool live = i < n;
  const float2 yi = live ? y[i] : make_float2(0.f, 0.f);
  float sq = 0.f, sx = 0.f, sy = 0.f;
  const int c_lo = slice * cps, c_hi = min(chunks, c_lo + cps);
  for (int c = c_lo; c < c_hi; ++c) {               // bound: cps chunks (none for an empty slice)
    const int j0 = c * TC, cnt = min(TC, n - j0);
    __syncthreads();                                // the readers of the chunk before are done
    for (int t = tid; t < cnt; t += TT) pts[t] = y[j0 + t];                  // bound: TC / TT trips
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) {              // bound: at most TC points, rising j
      const float2 yj = pts[jj];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float d2 = fmaf(dy, dy, dx * dx);
      float q = __builtin_amdgcn_rcpf(1.f + d2);
      q = (j0 + jj == i) ? 0.f : q;                 // the self pair, by index
      const float q2 = q * q;
      sq += q;
      sx = fmaf(q2, dx, sx);
      sy = fmaf(q2, dy, sy);
    }
  }
  if (live) ws[(int64_t)i * S + slice] = make_float4(sq, sx, sy, 0.f);
}

// one workgroup: thread t takes the partials t, t + TSNE_FOLD, ... in float64, then the tree
__global__ __launch_bounds__(TSNE_FOLD) void tsne_zfold_kernel(const float4* ws, int64_t count, double* Z) {
  __shared__ double sh[TSNE_FOLD];
  double s = 0.0;
  for (int64_t t = threadIdx.x; t < count; t += TSNE_FOLD) s += (double)ws[t].x;   // bound: ceil(n S / 1024) per thread
  s = block_sum(s, sh);
  if (threadIdx.x == 0) Z[0] = s;
}

const char* tsne_plan(int n, int slices_hint, TsnePlan* out) {
  if (n < 2 || n > SSLCR_TSNE_MAX_N) return "n outside [2, 2^20]";
  if (slices_hint < 0) return "slices < 0";
  const int row_tiles = (n + TT - 1) / TT, chunks = (n + TC - 1) / TC;
  int S = slices_hint > 0 ? slices_hint : (TSNE_FILL + row_tiles - 1) / row_tiles;
  if (S > SSLCR_TSNE_MAX_SLICES) S = SSLCR_TSNE_MAX_SLICES;
  if (S > chunks) S = chunks;
  const int cps = (chunks + S - 1) / S;
  if (slices_hint == 0) S = (chunks + cps - 1) / cps;                        // the plan's own choice leaves no slice empty
  out->tile = TT; out->chunk = TC;
  out->slices = S;
  out->chunks_per_slice = cps;
  out->grid[0] = row_tiles * S;
  out->grid[1] = 1;
  out->grid[2] = (n + 3) / 4;
  out->lds_bytes = sizeof(float2) * TC;
  out->workspace_bytes = (size_t)n * (size_t)S * sizeof(float4);
  return nullptr;
}

hipError_t launch_tsne_repulsion(const sslcr_tsne_grad_desc& a, const TsnePlan& p, hipStream_t st) {
  const int row_tiles = p.grid[0] / p.slices, chunks = (a.n + TC - 1) / TC;
  hipLaunchKernelGGL(tsne_repulsion_kernel, dim3((unsigned)row_tiles, (unsigned)p.slices), dim3(TT), 0, st,
                     reinterpret_cast<const float2*>(a.y), static_cast<float4*>(a.workspace), a.n, p.slices, chunks, p.chunks_per_slice);
  hipLaunchKernelGGL(tsne_zfold_kernel, dim3(1), dim3(TSNE_FOLD), 0, st, static_cast<const float4*>(a.workspace),
                     (int64_t)a.n * p.slices, a.Z);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 4. gradient and update
__global__ __launch_bounds__(256) void tsne_update_kernel(const sslcr_tsne_grad_desc a, int S) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n) return;                           // wave-uniform
  const float2* y = reinterpret_cast<const float2*>(a.y);
  const float2 yi = y[row];
  const double yix = (double)yi.x, yiy = (double)yi.y;
  const double Z = a.Z[0];
  // the repulsive partials: lane s holds slice s, folded in rising s
  const float4* ws = static_cast<const float4*>(a.workspace);
  const float4 part = lane < S ? ws[(int64_t)row * S + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
  double rx = 0.0, ry = 0.0;
  for (int s = 0; s < S; ++s) {                     // bound: S <= 64 slices
    rx += (double)__shfl(part.y, s);
    ry += (double)__shfl(part.z, s);
  }
  // the attractive sum over the row's CSR entries (a hub row has up to n - 1): lanes stride, then the butterfly
  int lo = a.rowptr[row], hi = a.rowptr[row + 1];
  if (lo < 0) lo = 0;
  if (hi > a.nnz) hi = a.nnz;
  double ax = 0.0, ay = 0.0, kl = 0.0;
  for (int e = lo + lane; e < hi; e += 64) {        // bound: ceil((hi - lo) / 64) entries per lane, rising e
    const int j = a.col[e];
    if ((unsigned)j >= (unsigned)a.n) continue;
    const double p = (double)a.val[e];
    const float2 yj = y[j];
    const double dx = yix - (double)yj.x, dy = yiy - (double)yj.y;
    const double q = 1.0 / (1.0 + (dx * dx + dy * dy));
    const double pq = p * q;
    ax += pq * dx;
    ay += pq * dy;
    if (a.kl_rows && p > 0.0) kl += p * log(p / fmax(q / Z, DBL_EPSILON));
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if (a.kl_rows) {
    kl = wave_sum(kl);
    if (lane == 0) a.kl_rows[row] = kl;
  }
  if (lane >= 2) return;
  // lane 0: x, lane 1: y
  const double g = 4.0 * (a.exaggeration * (lane ? ay : ax) - (lane ? ry : rx) / Z);
  const int64_t at = (int64_t)row * 2 + lane;
  a.grad[at] = (float)g;
  if (!a.y_out) return;
  const double up = (double)a.update[at], ga = (double)a.gains[at];
  const bool inc = up * g < 0.0;
  const float gain = (float)fmax(inc ? ga + 0.2 : ga * 0.8, a.min_gain);
  const float nu = (float)(a.momentum * up - a.lr * (double)gain * g);
  a.gains[at] = gain;
  a.update[at] = nu;
  a.y_out[at] = (float)((lane ? yiy : yix) + (double)nu);
}

hipError_t launch_tsne_update(const sslcr_tsne_grad_desc& a, const TsnePlan& p, hipStream_t st) {
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)p.grid[2]), dim3(256), 0, st, a, p.slices);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 5. the log row
__global__ __launch_bounds__(TSNE_FOLD) void tsne_kl_kernel(const double* kl_rows, const float* grad, const double* Z, double* log_row, int n,
                                                             int iteration) {
  __shared__ double sh[TSNE_FOLD];
  double k = 0.0, g = 0.0;
  for (int t = threadIdx.x; t < n; t += TSNE_FOLD) k += kl_rows[t];          // bound: ceil(n / 1024) per thread
  for (int t = threadIdx.x; t < 2 * n; t += TSNE_FOLD) {                     // bound: ceil(2 n / 1024) per thread
    const double v = (double)grad[t];
    g += v * v;
  }
  k = block_sum(k, sh);
  g = block_sum(g, sh);
  if (threadIdx.x == 0) {
    log_row[0] = k;
    log_row[1] = sqrt(g);
    log_row[2] = Z[0];
    log_row[3] = (double)iteration;
  }
}

hipError_t launch_tsne_kl(const double* kl_rows, const float* grad, const double* Z, double* log_row, int n, int iteration, hipStream_t st) {
  hipLaunchKernelGGL(tsne_kl_kernel, dim3(1), dim3(TSNE_FOLD), 0, st, kl_rows, grad, Z, log_row, n, iteration);
  return hipGetLastError();
}

}  // namespace sslcr
