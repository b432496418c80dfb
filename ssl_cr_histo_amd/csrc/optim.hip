// Fused multi-tensor optimizers, Lookahead/EMA axpby and weight packing (incl. eval-mode BN folding).
// Replaces torch.optim.Adam / SGD(nesterov) per-tensor kernel storms, Lookahead (lookahead.py:81-106),
// teacher refresh (K15) and prepares the KRSC / CRSK shadow weights the conv kernels consume.
#include "kernels.hpp"

namespace sslcr {

// The kernels take the optimizer rows BY VALUE (OptTable: up to SSLCR_MAX_OPT_GROUPS parameter groups); a tensor's row is
// row[TensorDesc.group].  A workgroup serves one tensor, so the row and the effective gradient scale are wave-uniform: they are
// read once per workgroup into scalar registers and the per-element arithmetic is what it was with a single sslcr_opt_desc.
struct OptRow {
  OptArgs o;
  float gs;     // grad_scale, times the clipping coefficient where one is given
  float keep;   // AdamW: 1 - lr * wd
};
// a wave-uniform float back into a scalar register (gfx950 has no scalar float ALU: the product would otherwise occupy a VGPR)
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ OptRow opt_row(const OptTable& tab, int group, const float* __restrict__ coef) {
  OptRow r;
  r.o = tab.row[group & (SSLCR_MAX_OPT_GROUPS - 1)];
  r.gs = coef ? uniform(r.o.grad_scale * coef[0]) : r.o.grad_scale;
  r.keep = uniform(1.f - r.o.lr * r.o.wd);
  return r;
}

// one parameter element: i indexes p / s1 / s2, gi the gradient.  Returns the new value.
__device__ __forceinline__ float opt_update_g(const TensorDesc& d, const OptRow& r, int i, float graw);
__device__ __forceinline__ float opt_update(const TensorDesc& d, const OptRow& r, int i, int gi) {
  return opt_update_g(d, r, i, d.g[gi]);
}
// ... with the raw gradient element already in hand
__device__ __forceinline__ float opt_update_g(const TensorDesc& d, const OptRow& r, int i, float graw) {
  const OptArgs& o = r.o;
  float p = d.p[i];
  float g;
  if (o.kind == 2) {                  // AdamW: decoupled decay first (torch: param.mul_(1 - lr * weight_decay)), no wd in the gradient
    p *= r.keep;
    g = graw * r.gs;
  } else {
    g = fmaf(o.wd, p, graw * r.gs);
  }
  if (o.kind != 1) {                  // Adam (0: L2 decay in the gradient) / AdamW (2), eps outside the sqrt
    float m = d.s1[i], v = d.s2[i];
    m = fmaf(o.beta1, m, (1.f - o.beta1) * g);
    v = fmaf(o.beta2, v, (1.f - o.beta2) * g * g);
    d.s1[i] = m;
    d.s2[i] = v;
    const float denom = sqrtf(v) / sqrtf(o.bc2) + o.eps;
    p -= (o.lr / o.bc1) * (m / denom);
  } else {                            // SGD momentum, nesterov
    float buf = o.first_step ? g : fmaf(o.momentum, d.s1[i], g);
    d.s1[i] = buf;
    p -= o.lr * fmaf(o.momentum, buf, g);
  }
  d.p[i] = p;
  return p;
}
__device__ __forceinline__ void opt_pack(const TensorDesc& d, int k, int c, int rs, int gi, float p) {
  if (d.w_fwd) {
    if (d.pack_dtype == DT_BF16) Elem<bf16_t>::st(reinterpret_cast<bf16_t*>(d.w_fwd) + gi, p);
    else reinterpret_cast<float*>(d.w_fwd)[gi] = p;
  }
  if (d.w_dgrad) {
    const size_t o = ((size_t)c * d.RS + (d.dgrad_flip ? d.RS - 1 - rs : rs)) * d.K + k;
    if (d.pack_dtype == DT_BF16) Elem<bf16_t>::st(reinterpret_cast<bf16_t*>(d.w_dgrad) + o, p);
    else reinterpret_cast<float*>(d.w_dgrad)[o] = p;
  }
}

// generic form (sslcr_optimizer_step): a fixed number of workgroups per tensor
__global__ __launch_bounds__(256) void optimizer_kernel(const TensorDesc* __restrict__ descs, const OptTable tab,
                                                        const float* __restrict__ coef) {
  const TensorDesc d = descs[blockIdx.y];
  const OptRow o = opt_row(tab, d.group, coef);
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += stride) {
    int gi = i, k = 0, c = 0, rs = 0;
    if (d.K > 0) {                      // param [K][C][RS]  <-  grad [K][RS][C]
      const int crs = d.C * d.RS;
      k = i / crs;
      const int rem = i - k * crs;
      c = rem / d.RS; rs = rem - c * d.RS;
      gi = (k * d.RS + rs) * d.C + c;
    }
    const float p = opt_update(d, o, i, gi);
    if (d.K > 0) opt_pack(d, k, c, rs, gi, p);
  }
}

hipError_t launch_optimizer(const TensorDesc* d_descs, int ntensors, int max_n, const OptTable& tab, const float* coef, hipStream_t st) {
  int bx = cdiv(max_n, 256 * 8);
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(optimizer_kernel, dim3(bx, ntensors), dim3(256), 0, st, d_descs, tab, coef);
  return hipGetLastError();
}

// engine form: a work list of chunks, so that the four 2.4 M-element layer4 filters (85 % of the parameters) get 85 % of the
// workgroups instead of 64 each.  Chunks run in PARAMETER order (p, s1, s2 coalesced; the gradient gather and the two
// bf16 shadow-weight writes are the strided streams).  Gradient order -- one output channel per chunk, c fastest -- was
// measured 0.3 ms/step slower: the 36-byte stride it puts on the three fp32 state arrays costs more than it saves.
// The shadow weights of the updated value are written here, which removes the 19 pack launches that followed every step
// (step 20.33 -> 20.24 ms).
// (waves_per_eu 5: the register allocator otherwise settles on 98 VGPRs -- one 8-register granule above the 96 that five waves per
// SIMD allow, which is where this kernel ran before the group table; with the hint it takes 95 and no scratch)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void optimizer_chunks_kernel(const TensorDesc* __restrict__ descs, const int2* __restrict__ chunks,
                                                               const OptTable tab, const float* __restrict__ coef) {
  // chunk.x = tensor | group << OPT_CHUNK_GROUP_SHIFT: the work list repeats the tensor's group so that the row's scalar loads do
  // not wait for the descriptor's (descriptor -> group -> row would be one more dependent load in front of every workgroup)
  const int2 ch = chunks[blockIdx.x];
  const TensorDesc d = descs[ch.x & ((1 << OPT_CHUNK_GROUP_SHIFT) - 1)];
  const OptRow o = opt_row(tab, ch.x >> OPT_CHUNK_GROUP_SHIFT, coef);
  if (ch.y < 0) {
    // 3x3 filter with shadow weights, tile (16 kout) x (16 cin) x 9 taps = 2304 elements through LDS, so that EVERY stream is
    // a run of >= 32 bytes: gradient [K][9][C] in (64-byte runs of 16 cin), parameter / moments [K][C][9] (576-byte runs),
    // forward weights [K][9][C] and dgrad weights [C][9][K] out (32-byte runs).  In parameter order three of the five
    // streams were 2- and 4-byte accesses a filter row apart (the kernel ran at 1.6 TB/s).
    __shared__ float sm[16 * 145];               // parameter order, one pad word per kout: kl * 145 + cl * 9 + rs
    const int tile = -ch.y - 1, ctiles = d.C / 16;
    const int k0 = (tile / ctiles) * 16, c0 = (tile % ctiles) * 16;
#pragma unroll
    for (int j = 0; j < OPT_TILE / 256; ++j) {     // gradient order in
      const int e = threadIdx.x + 256 * j;
      const int cl = e & 15, t2 = e >> 4, kl = t2 / 9, rs = t2 - kl * 9;
      sm[kl * 145 + cl * 9 + rs] = d.g[((size_t)(k0 + kl) * 9 + rs) * d.C + c0 + cl];
    }
    __syncthreads();
    float pv[OPT_TILE / 256];
#pragma unroll
    for (int j = 0; j < OPT_TILE / 256; ++j) {     // parameter order: the update
      const int e = threadIdx.x + 256 * j;
      const int kl = e / 144, rem = e - kl * 144;
      pv[j] = opt_update_g(d, o, ((k0 + kl) * d.C + c0) * 9 + rem, sm[e + kl]);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < OPT_TILE / 256; ++j) { const int e = threadIdx.x + 256 * j; sm[e + e / 144] = pv[j]; }
    __syncthreads();
    const bool bf = d.pack_dtype == DT_BF16;
#pragma unroll
    for (int j = 0; j < OPT_TILE / 256; ++j) {     // forward weights out: [k][rs][c]
      const int e = threadIdx.x + 256 * j;
      const int cl = e & 15, t2 = e >> 4, kl = t2 / 9, rs = t2 - kl * 9;
      const float p = sm[kl * 145 + cl * 9 + rs];
      const size_t oo = ((size_t)(k0 + kl) * 9 + rs) * d.C + c0 + cl;
      if (bf) Elem<bf16_t>::st(reinterpret_cast<bf16_t*>(d.w_fwd) + oo, p);
      else reinterpret_cast<float*>(d.w_fwd)[oo] = p;
    }
#pragma unroll
    for (int j = 0; j < OPT_TILE / 256; ++j) {     // dgrad weights out: [c][rs'][k]
      const int e = threadIdx.x + 256 * j;
      const int kl = e & 15, t2 = e >> 4, cl = t2 / 9, rs = t2 - cl * 9;
      const float p = sm[kl * 145 + cl * 9 + rs];
      const size_t oo = ((size_t)(c0 + cl) * 9 + (d.dgrad_flip ? 8 - rs : rs)) * d.K + k0 + kl;
      if (bf) Elem<bf16_t>::st(reinterpret_cast<bf16_t*>(d.w_dgrad) + oo, p);
      else reinterpret_cast<float*>(d.w_dgrad)[oo] = p;
    }
  } else if (d.K > 0) {
    // parameter order (p, s1, s2 coalesced); the gradient gather and the two shadow-weight writes are the strided streams
    const int crs = d.C * d.RS;
    const int end = ch.y + OPT_CHUNK < d.n ? ch.y + OPT_CHUNK : d.n;
    for (int i = ch.y + threadIdx.x; i < end; i += 256) {
      const int k = i / crs, rem = i - k * crs;
      const int c = rem / d.RS, rs = rem - c * d.RS;
      const int gi = (k * d.RS + rs) * d.C + c;
      opt_pack(d, k, c, rs, gi, opt_update(d, o, i, gi));
    }
  } else {
    const int end = ch.y + OPT_CHUNK < d.n ? ch.y + OPT_CHUNK : d.n;
    for (int i = ch.y + threadIdx.x; i < end; i += 256) opt_update(d, o, i, i);
  }
}
hipError_t launch_optimizer_chunks(const TensorDesc* d_descs, const void* d_chunks, int nchunks, const OptTable& tab, const float* coef,
                                   hipStream_t st) {
  if (nchunks < 1) return hipSuccess;
  hipLaunchKernelGGL(optimizer_chunks_kernel, dim3(nchunks), dim3(256), 0, st, d_descs, reinterpret_cast<const int2*>(d_chunks), tab, coef);
  return hipGetLastError();
}

// ------------------------------------------------------------------ global gradient norm (torch.nn.utils.clip_grad_norm_)
// Deterministic and without atomics: GRAD_NORM_BLOCKS workgroups, each owning one fixed contiguous slice of the buffer.  The
// slices are cut on 16-byte boundaries of the ADDRESS: the up-to-3 elements in front of the first boundary (any 4-byte-aligned
// base is served) go to workgroup 0 as scalars, every slice is then a whole number of float4 quads, and the up-to-3 elements
// behind the last whole quad go to the workgroup that owns them as scalars.  A thread walks its quads in a fixed order and
// accumulates (double)g * (double)g -- exact: 48 significand bits -- in double; the block fold is a fixed tree.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partials) {
  __shared__ double red[256];
  size_t head = ((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) / 4;
  if (head > n) head = n;
  const size_t quads = (n - head) / 4;                                     // whole aligned quads behind the head
  const size_t per = (quads + GRAD_NORM_BLOCKS - 1) / GRAD_NORM_BLOCKS;    // quads per workgroup
  size_t q0 = per * blockIdx.x, q1 = q0 + per;
  if (q0 > quads) q0 = quads;
  if (q1 > quads) q1 = quads;
  const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
  double acc = 0.0;
  for (size_t q = q0 + threadIdx.x; q < q1; q += 256) {
    const float4 v = gv[q];
    acc = fma((double)v.x, (double)v.x, acc);
    acc = fma((double)v.y, (double)v.y, acc);
    acc = fma((double)v.z, (double)v.z, acc);
    acc = fma((double)v.w, (double)v.w, acc);
  }
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0)
      for (size_t i = 0; i < head; ++i) acc = fma((double)g[i], (double)g[i], acc);
    // the tail belongs to the workgroup whose slice ends the quads (the last one with work, or workgroup 0 when there are none)
    const size_t owner = quads == 0 ? 0 : (quads - 1) / per;
    if (blockIdx.x == owner)
      for (size_t i = head + quads * 4; i < n; ++i) acc = fma((double)g[i], (double)g[i], acc);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}
// one workgroup: thread t folds partials [4t, 4t + 4) in index order, the 256 results fold in the same fixed tree;
// out2 = {norm, coef} with torch's clip_grad_norm_ arithmetic: coef = min(1, max_norm / (norm + 1e-6))
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ partials, float max_norm, float* __restrict__ out2) {
  __shared__ double red[256];
  constexpr int PER = GRAD_NORM_BLOCKS / 256;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) acc += partials[threadIdx.x * PER + j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    out2[0] = norm;
    // (a NaN norm gives coef 1 here -- fminf returns its other operand -- where torch's clamp keeps NaN; the NaN gradients reach
    // the parameters either way)
    out2[1] = fminf(1.f, max_norm / (norm + 1e-6f));
  }
}
hipError_t launch_grad_norm(const float* g, size_t n, float max_norm, double* partials, float* out2, hipStream_t st) {
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GRAD_NORM_BLOCKS), dim3(256), 0, st, g, n, partials);
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, st, partials, max_norm, out2);
  return hipGetLastError();
}

// ------------------------------------------------------------------ gradient accumulation (autograd's `.grad +=`)
// dst[i] = dst[i] + src[i]: one fp32 add per element, nothing to contract or reassociate, no LDS, no atomics -- every element has one
// writer, so the bits are the same on every run and on every rank that holds the same two buffers.  Cut as grad_sumsq_kernel cuts its
// buffer, on 16-byte boundaries of the DESTINATION address: the up-to-3 elements in front of the first boundary and the up-to-3
// behind the last whole quad are scalars of workgroup 0, the body is whole float4 quads walked with a grid stride (the
// elementwise family's grid: launch_grad_accumulate).  dst and src may sit at different offsets mod 16: the source quad is then
// only 4-byte aligned, which global_load_dwordx4 serves (its type says so; the destination's load and store are aligned).
typedef float f32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  size_t head = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / 4;
  if (head > n) head = n;
  const size_t quads = (n - head) / 4;                                     // whole destination-aligned quads behind the head
  float4* __restrict__ dv = reinterpret_cast<float4*>(dst + head);
  const f32x4_a4_t* __restrict__ sv = reinterpret_cast<const f32x4_a4_t*>(src + head);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) {
    float4 a = dv[q];
    const f32x4_a4_t b = __builtin_nontemporal_load(sv + q);               // read once; the sum is what the optimizer reads next
    a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
    dv[q] = a;
  }
  if (blockIdx.x == 0) {
    const size_t t = threadIdx.x, tail0 = head + quads * 4;
    if (t < head) dst[t] = dst[t] + src[t];
    if (tail0 + t < n) dst[tail0 + t] = dst[tail0 + t] + src[tail0 + t];
  }
}
hipError_t launch_grad_accumulate(float* dst, const float* src, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  // three workgroups per CU at most, as bn_eltwise.hip's ew_grid(): one quad per thread and trip
  const size_t cap = 3 * (size_t)device_cus();
  size_t b = (n / 4 + 255) / 256;
  b = b < 1 ? 1 : (b > cap ? cap : b);
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((int)b), dim3(256), 0, st, dst, src, n);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void axpby_kernel(float* p, float* q, size_t n, float alpha, int copy_back) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = alpha * p[i] + (1.f - alpha) * q[i];
    p[i] = v;
    if (copy_back) q[i] = v;
  }
}
hipError_t launch_axpby(float* p, float* q, size_t n, float alpha, int copy_back, hipStream_t st) {
  size_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(axpby_kernel, dim3((int)b), dim3(256), 0, st, p, q, n, alpha, copy_back);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void fill_kernel(float* p, size_t n, float v) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t st) {
  size_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(fill_kernel, dim3((int)b), dim3(256), 0, st, p, n, v);
  return hipGetLastError();
}

// ------------------------------------------------------------------ weight packing
template <typename T>
__global__ __launch_bounds__(256) void pack_conv_kernel(const PackArgs a) {
  const int RS = a.R * a.S;
  const int total = a.K * a.C * RS;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    // i enumerates the fwd layout [K][RS][C]
    const int k = i / (RS * a.C), rem = i - k * RS * a.C;
    const int rs = rem / a.C, c = rem - rs * a.C;
    const float w = a.w[((size_t)k * a.C + c) * RS + rs];
    if (a.w_fwd) {
      float f = 1.f;
      if (a.gamma && !a.scale_out) f = a.gamma[k] / sqrtf(a.rvar[k] + a.eps);      // (scale_out: the scale goes to the conv's epilogue)
      Elem<T>::st(reinterpret_cast<T*>(a.w_fwd) + i, w * f);
    }
    if (a.w_dgrad) Elem<T>::st(reinterpret_cast<T*>(a.w_dgrad) + ((size_t)c * RS + (a.dgrad_flip ? RS - 1 - rs : rs)) * a.K + k, w);
  }
  if (a.gamma && a.bias_out) {
    for (int k = blockIdx.x * 256 + threadIdx.x; k < a.K; k += gridDim.x * 256) {
      const float f = a.gamma[k] / sqrtf(a.rvar[k] + a.eps);
      a.bias_out[k] = a.beta[k] - a.rmean[k] * f;
      if (a.scale_out) a.scale_out[k] = f;
    }
  }
}
hipError_t launch_pack_conv(int dtype, const PackArgs& a, hipStream_t st) {
  int b = cdiv(a.K * a.C * a.R * a.S, 256);
  if (b > 2048) b = 2048;
  if (dtype == DT_BF16) {
    hipLaunchKernelGGL(pack_conv_kernel<bf16_t>, dim3(b), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(pack_conv_kernel<float>, dim3(b), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

// stem: [64][3][7][7] -> [64][7][8][4] (s = 7 and c = 3 are zero padding of the MFMA K dimension)
template <typename T>
__global__ __launch_bounds__(256) void pack_stem_kernel(const PackArgs a) {
  const int total = 64 * 7 * 8 * 4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c = i & 3, s = (i >> 2) & 7, r = (i >> 5) % 7, k = i / 224;
    float w = 0.f;
    if (c < 3 && s < 7) {
      w = a.w[((k * 3 + c) * 7 + r) * 7 + s];
      if (a.gamma && !a.scale_out) w *= a.gamma[k] / sqrtf(a.rvar[k] + a.eps);
    }
    Elem<T>::st(reinterpret_cast<T*>(a.w_fwd) + i, w);
  }
  if (a.gamma && a.bias_out && blockIdx.x == 0 && threadIdx.x < 64) {
    const int k = threadIdx.x;
    const float f = a.gamma[k] / sqrtf(a.rvar[k] + a.eps);
    a.bias_out[k] = a.beta[k] - a.rmean[k] * f;
    if (a.scale_out) a.scale_out[k] = f;
  }
}
hipError_t launch_pack_stem(int dtype, const PackArgs& a, hipStream_t st) {
  if (dtype == DT_BF16) {
    hipLaunchKernelGGL(pack_stem_kernel<bf16_t>, dim3(56), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(pack_stem_kernel<float>, dim3(56), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace sslcr

namespace sslcr {

// dst[r*ldd + c] (+)= src[r*lds + c], c < w   (concat / tile / slice-sum glue for the fp32 heads)
__global__ __launch_bounds__(256) void copy2d_kernel(float* dst, long ldd, const float* src, long lds, int rows, int w, int accumulate) {
  const long total = (long)rows * w;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / w, c = i - r * w;
    const float v = src[r * lds + c];
    float* d = dst + r * ldd + c;
    *d = accumulate ? *d + v : v;
  }
}
// dst[j*dstep + r*ldd + c] = sum_i src[i*sstep + r*lds + c] for j < ndst, i < nsrc, left to right: the tile ([f, f, f],
// [E, E]) and slice-sum (their gradients) forms of the single-branch head in ONE launch each instead of two or three
__global__ __launch_bounds__(256) void copy2d_multi_kernel(float* dst, long ldd, int ndst, long dstep, const float* src, long lds, int nsrc,
                                                           long sstep, int rows, int w) {
  const long total = (long)rows * w;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / w, c = i - r * w;
    float v = src[r * lds + c];
    for (int s = 1; s < nsrc; ++s) v += src[s * sstep + r * lds + c];
    for (int j = 0; j < ndst; ++j) dst[j * dstep + r * ldd + c] = v;
  }
}
hipError_t launch_copy2d_multi(float* dst, long ldd, int ndst, long dstep, const float* src, long lds, int nsrc, long sstep, int rows, int w,
                               hipStream_t st) {
  long b = ((long)rows * w + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(copy2d_multi_kernel, dim3((int)b), dim3(256), 0, st, dst, ldd, ndst, dstep, src, lds, nsrc, sstep, rows, w);
  return hipGetLastError();
}
hipError_t launch_copy2d(float* dst, long ldd, const float* src, long lds, int rows, int w, int accumulate, hipStream_t st) {
  long b = ((long)rows * w + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(copy2d_kernel, dim3((int)b), dim3(256), 0, st, dst, ldd, src, lds, rows, w, accumulate);
  return hipGetLastError();
}

// engine gradient layout [K][RS][C] -> PyTorch [K][C][RS]
__global__ __launch_bounds__(256) void unpack_grad_kernel(const float* g, float* out, int K, int C, int RS) {
  const int total = K * C * RS;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i / (C * RS), rem = i - k * C * RS;
    const int c = rem / RS, rs = rem - c * RS;
    out[i] = g[(k * RS + rs) * C + c];
  }
}
hipError_t launch_unpack_grad(const float* g, float* out, int K, int C, int RS, hipStream_t st) {
  int b = cdiv(K * C * RS, 256);
  if (b > 2048) b = 2048;
  hipLaunchKernelGGL(unpack_grad_kernel, dim3(b), dim3(256), 0, st, g, out, K, C, RS);
  return hipGetLastError();
}

}  // namespace sslcr
