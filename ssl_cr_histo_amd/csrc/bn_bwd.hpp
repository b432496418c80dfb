// What the BatchNorm-backward kernels of bn_eltwise.hip (bn_bwd_reduce* / bn_bwd_apply* / bn_param_grads_kernel) and the fused stem
// weight-gradient kernels of stem.hip (stem_wgrad_kernel<POOL>, stem_wgrad_pool2_kernel) share: each piece of their arithmetic once.
// The float64 tests bound these expressions operation by operation (tests/_f64.py): the order of the floating-point operations
// below is part of the interface.  Device-only, no launchers.
#pragma once
#include "kernels.hpp"

namespace sslcr {

// dx = cA*g + cB*x + cC with cA = scale, cB = -scale*invstd^2*mean(g*(x-mu)), cC = -scale*mean(g) - cB*mu, for the thread's NCH
// channels cb .. cb + NCH - 1 of a BatchNorm over C channels (a.sums = [2][C]: sum g, sum g*(x-mu)).  cA is also the scale of
// relu_from_x's bn(x) > 0 test; the shift that goes with it stays at the caller.
template <int NCH>
__device__ __forceinline__ void bn_bwd_coeffs(const BnBwdArgs& a, int C, int cb, float (&cA)[NCH], float (&cB)[NCH], float (&cC)[NCH]) {
  const float invM = (float)(1.0 / a.count);
#pragma unroll
  for (int e = 0; e < NCH; ++e) {
    const int c = cb + e;
    const float is = a.invstd[c], sc = a.scale[c];
    const float m0 = (float)a.sums[c] * invM, m1 = (float)a.sums[C + c] * invM;
    cA[e] = sc;
    cB[e] = -sc * is * is * m1;
    cC[e] = -sc * m0 - cB[e] * a.mean[c];
  }
}

// affine gradients of channel c from the finished sums ([2][C]): float += (float)(double product), the same bits wherever they are
// formed -- bn_param_grads_kernel, workgroup 0 of an apply pass (bn_bwd_param_grads) or of a fused stem weight-gradient kernel
// (tests: test_bn_param_grads_one_arithmetic)
__device__ __forceinline__ void bn_bwd_affine_grads(float& dgamma, float& dbeta, const double* sums, const float* invstd, int C, int c, float pg_scale) {
  dgamma += (float)(sums[C + c] * (double)invstd[c] * (double)pg_scale);
  dbeta += (float)(sums[c] * (double)pg_scale);
}

// End of a reduce workgroup of NB threads: sm[thread][which * EPC + e] holds the thread's NW partial sums of its EPC channels
// (thread = pixel row rl * cols + column); thread t < cols * NW * EPC adds one (column, which, e) over the rpp pixel rows in rising
// order, in fp64, and hands the sum to put(which, channel, sum) -- the caller's row addressing.
template <int NW, int EPC, int NB, typename Put>
__device__ __forceinline__ void bn_bwd_fold_columns(const float (*sm)[NW * EPC + 1], int cols, int rpp, Put put) {
  for (int t = threadIdx.x; t < cols * NW * EPC; t += NB) {
    const int cc = t / (NW * EPC), q = t - cc * NW * EPC;
    double acc = 0.0;
    for (int r = 0; r < rpp; ++r) acc += (double)sm[r * cols + cc][q];
    const int which = q / EPC, e = q - which * EPC;
    put(which, cc * EPC + e, acc);
  }
}

// ---- the gradient through the stem's 3x3/2 pad-1 max-pool (pool_dy + one argmax byte per pooled element, sslcr_bn_bwd_desc): the
// un-pooled gradient tensor is never materialised.
// The four windows (oh0 + (k >> 1), ow0 + (k & 1)), k = 0..3, of image n, 16-byte column col of cols: gradient chunk and the chunk's
// argmax bytes.  All four are loaded UNCONDITIONALLY (clamped addresses) so the loads go out back to back; a window outside the
// pooled map is then dropped by the caller's select -- no divergent branches around memory operations.
template <typename T, bool NT>
__device__ __forceinline__ void bn_pool_windows(const BnBwdArgs& a, size_t n, int oh0, int ow0, int cols, int col, u32x4_t (&dv)[4], uint32_t (&am)[4][2]) {
  constexpr int EPC = Elem<T>::EPC;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int oh = oh0 + (k >> 1), ow = ow0 + (k & 1);
    const int ohc = oh < a.pOH ? oh : a.pOH - 1, owc = ow < a.pOW ? ow : a.pOW - 1;
    const size_t o = ((n * a.pOH + ohc) * a.pOW + owc) * cols + col;
    const char* p = reinterpret_cast<const char*>(a.pool_dy) + o * 16;
    dv[k] = NT ? ld16_nt(p) : ld16(p);
    if constexpr (EPC == 8) { const u32x2_t v = *reinterpret_cast<const u32x2_t*>(a.pool_argmax + o * EPC); am[k][0] = v[0]; am[k][1] = v[1]; }
    else { am[k][0] = *reinterpret_cast<const uint32_t*>(a.pool_argmax + o * EPC); am[k][1] = 0; }
  }
}
// argmax code of element e of a chunk: (row * 3 + column) of the maximum inside its 3x3 window, 9 = nobody
__device__ __forceinline__ uint32_t bn_pool_code(const uint32_t (&am)[2], int e) { return (am[e >> 2] >> (8 * (e & 3))) & 0xffu; }
// a loaded window as bn_pool_gather takes it: its gradients as floats, ZERO where the window lies outside the pooled map (!wok:
// the clamped address held somebody else's), and its decoded codes
template <typename T>
__device__ __forceinline__ void bn_pool_decode(u32x4_t v, const uint32_t (&am)[2], bool wok, float (&dw)[Elem<T>::EPC], uint32_t (&cd)[Elem<T>::EPC]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = wok ? v[j] : 0u;
  Elem<T>::unpack(v, dw);
#pragma unroll
  for (int e = 0; e < Elem<T>::EPC; ++e) cd[e] = bn_pool_code(am, e);
}

// 2x2 input-pixel blocks: the four pixels (2a+pi, 2b+pj) share the four pooling windows (a+di, b+dj), and the argmax code a window
// must carry to select pixel (pi, pj) is a compile-time constant (pi - 2di + 1) * 3 + (pj - 2dj + 1) once the caller's pixel loops
// are unrolled.  g = pixel (pi, pj)'s gradient; dw[di * 2 + dj] / cd[di * 2 + dj] = window (di, dj)'s gradients (ZERO where the
// window lies outside the pooled map) and decoded codes.  Branch-free: the argmax match is a select.
template <int N>
__device__ __forceinline__ void bn_pool_gather(int pi, int pj, const float (&dw)[4][N], const uint32_t (&cd)[4][N], float (&g)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) g[e] = 0.f;
#pragma unroll
  for (int di = 0; di <= pi; ++di)
#pragma unroll
    for (int dj = 0; dj <= pj; ++dj) {
      const uint32_t code = (uint32_t)((pi - 2 * di + 1) * 3 + (pj - 2 * dj + 1));
#pragma unroll
      for (int e = 0; e < N; ++e) g[e] += cd[di * 2 + dj][e] == code ? dw[di * 2 + dj][e] : 0.f;
    }
}

}  // namespace sslcr
