// Linear probe over fixed features (include/sslcr.h has the contract and the definitions):
//   linprobe_pack    W [C][D] -> the zero-padded [16 CB][Dp] copy in the operand order of the first product
//   linprobe_kernel  per workgroup: a range of 32-row tiles; logits Z = X W^T + b, softmax / squared residual R, and the
//                    gradient R^T X kept in accumulators across the tiles -- X is fetched once per tile where the tile fits LDS
//   linprobe_fold    the per-workgroup partials folded in float64 in rising workgroup order, divided by the weight sum
// Both products run on v_mfma_f32_16x16x4_f32 as fmaf chains: the logit over d in rising order, the gradient over the workgroup's
// rows in rising order.  Work passes between workgroups at the launch boundary only: no kernel waits for another workgroup, there is
// no ticket and no floating-point atomic, and every loop states its bound.
#include "kernels.hpp"

namespace sslcr {

constexpr int LP_TM = SSLCR_LINPROBE_TILE, LP_KW = SSLCR_LINPROBE_CHUNK;
constexpr int LP_SC = 256;                          // columns per stage: one 16-byte piece a lane and row
constexpr int LP_ZP = SSLCR_LINPROBE_MAX_C + 4;     // floats per LDS row of the logit / residual tile
constexpr int LP_KS = LP_TM / 4;                    // row steps of the second product: 4 rows an MFMA
constexpr size_t LP_LDS_CAP = 160 * 1024;           // what one workgroup may declare
constexpr size_t LP_STAGED_MAX = 144 * 1024;        // a whole tile is staged up to this many bytes of LDS
static_assert(LP_TM == 32, "8 lanes a row in the residual pass; wave w owns row block w & 1 of the first product");
static_assert(LP_KW == 2 * LP_SC, "the streamed form alternates between two stages");

// floats per LDS row of the X tile for `cols` staged columns: = 20 mod 64, so that the 16 rows of a fragment read (16 bytes a lane)
// fall on 64 different banks, and the 4 rows of a second-product read overlap on 12 banks only
__host__ __device__ inline int lp_pitch(int cols) { return ((cols + 63) & ~63) + 20; }

struct LpGeom {
  int tiles, tpg;       // row tiles in all, and per workgroup
  int Dp;               // D padded to 16
  int streamed;         // the tile passes through LP_KW columns of LDS, twice
  int pitch;            // floats per LDS row of the X tile
};

// the repacked W: position 16 u + 4 g + e of a row holds element d = 16 u + 4 e + g, so that the ONE 16-byte load of lane (li, g) at
// 16 u + 4 g feeds MFMA e with d = 16 u + 4 e + g (lane group g is the k index of v_mfma_f32_16x16x4_f32): the X side reads the
// same elements from its natural-order tile
__host__ __device__ inline int lp_pos(int d) { return (d & ~15) + 4 * (d & 3) + ((d >> 2) & 3); }

// ------------------------------------------------------------------------------------------------ 0. repack W
__global__ __launch_bounds__(256) void linprobe_pack_kernel(const float* w, float* wp, int C, int D, int Dp, int rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * Dp) return;
  const int c = (int)(i / Dp), d = (int)(i - (int64_t)c * Dp);
  wp[(int64_t)c * Dp + lp_pos(d)] = (c < C && d < D) ? w[(int64_t)c * D + d] : 0.f;
}

// ------------------------------------------------------------------------------------------------ 1. value and gradient partials
// CB: class blocks of 16 (registers only); NB: 16 x 16 gradient blocks of columns a wave holds per class block.  Wave w of column
// slice s owns the column blocks s * 4 NB + w + 4 j, j < NB.
template <int CB, int NB, bool FWD_ONLY>
__global__ __launch_bounds__(256) void linprobe_kernel(const sslcr_linprobe_desc a, const float* wp, double* lossp, float* part, const LpGeom q) {
  extern __shared__ __attribute__((aligned(16))) float lp_lds[];
  float* xl = lp_lds;                               // [LP_TM][pitch]: the staged columns of the tile, in natural order
  float* zr = xl + LP_TM * q.pitch;                 // [LP_TM][LP_ZP]: logits, then residuals
  double* lt = reinterpret_cast<double*>(zr + LP_TM * LP_ZP);               // [LP_TM] s_i l_i
  double* lw = lt + LP_TM;                          // [LP_TM] s_i
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int D = a.D, C = a.C, Dp = q.Dp, pitch = q.pitch;
  const int grp = blockIdx.x, sl = blockIdx.y;
  const int t_lo = grp * q.tpg, t_hi = min(q.tiles, t_lo + q.tpg);
  const bool lead = sl == 0;                        // slice 0 writes logits, loss terms and the bias column
  constexpr int FC = (CB + 1) / 2;                  // class blocks of a wave in the first product: cb0, cb0 + 2
  const int rb = wave & 1, cb0 = wave >> 1;
  constexpr int CP = 16 * CB;

  f32x4_t acc[FWD_ONLY ? 1 : NB][CB];
#pragma unroll
  for (int j = 0; j < (FWD_ONLY ? 1 : NB); ++j)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[j][cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float gb = 0.f;                                   // wave 1, thread c: sum_i r_ic, one chain over the workgroup's rows
  double lsum = 0.0, wsum = 0.0;                    // wave 0: the workgroup's sums of s_i l_i and s_i

  // Staging, LP_SC columns at a time: one 16-byte piece a lane and row, a wave takes rows wave, wave + 4, ...  issue() starts the 8
  // loads of stage k into registers (rows past n and columns past D as zeros), commit() stores them -- in natural order, 16 bytes
  // a store -- once the stage's place in LDS is free.  The staged form keeps stage k at columns LP_SC k (the whole tile stays); the
  // streamed form alternates between the two halves of its LP_KW columns.  The loads of the NEXT stage (or of the next tile's first)
  // are in flight while this stage's MFMAs run.
  const int nsc = (Dp + LP_SC - 1) / LP_SC;
  const bool streamed = q.streamed != 0;
  auto col_off = [&](int k) { return streamed ? LP_SC * (k & 1) : LP_SC * k; };
  f32x4_t v[LP_TM / 4];
  auto issue = [&](int64_t r0, int k) {
    const int d = LP_SC * k + 4 * lane;
#pragma unroll
    for (int rr = 0; rr < LP_TM / 4; ++rr) {
      const int64_t row = r0 + wave + 4 * rr;
      v[rr] = (row < a.n && d < D) ? *reinterpret_cast<const f32x4_t*>(a.x + row * D + d) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto commit = [&](int k) {
    if (LP_SC * k + 4 * lane < Dp) {
#pragma unroll
      for (int rr = 0; rr < LP_TM / 4; ++rr) *reinterpret_cast<f32x4_t*>(xl + (wave + 4 * rr) * pitch + col_off(k) + 4 * lane) = v[rr];
    }
  };
  // the repacked W of UB groups of 16 columns, one batch ahead of the MFMAs that use it (batch gbi: groups UB gbi .. + UB - 1)
  constexpr int UB = FC == 1 ? 8 : 4;
  const float* wb = wp + (int64_t)(16 * cb0 + li) * Dp + 4 * g;
  const int ugroups = Dp >> 4;
  auto load_w = [&](f32x4_t (&dst)[UB][FC], int gbi) {
#pragma unroll
    for (int i = 0; i < UB; ++i)
#pragma unroll
      for (int fi = 0; fi < FC; ++fi) {
        const int u = UB * gbi + i;
        dst[i][fi] = (cb0 + 2 * fi < CB && u < ugroups) ? *reinterpret_cast<const f32x4_t*>(wb + (int64_t)32 * fi * Dp + 16 * u)
                                                         : f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
  };

  if (t_lo < t_hi) issue((int64_t)t_lo * LP_TM, 0);
  for (int t = t_lo; t < t_hi; ++t) {               // bound: tiles_per_group tiles, rising rows
    const int64_t r0 = (int64_t)t * LP_TM;
    // ---- first product: z = X W^T, wave (rb, cb0) owns rows 16 rb .. + 15 and class blocks cb0, cb0 + 2
    f32x4_t facc[FC];
#pragma unroll
    for (int i = 0; i < FC; ++i) facc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t fw[UB][FC], fwn[UB][FC];
    if (cb0 < CB) load_w(fw, 0);
    for (int k = 0; k < nsc; ++k) {                 // bound: ceil(Dp / 256) stages, rising d
      commit(k);
      if (k + 1 < nsc) issue(r0, k + 1);
      else if (streamed && !FWD_ONLY) issue(r0, 0);                          // the second pass over the tile
      else if (t + 1 < t_hi) issue(r0 + LP_TM, 0);
      __syncthreads();
      if (cb0 < CB) {                               // wave-uniform
        const int ucnt = min(LP_SC, Dp - LP_SC * k) >> 4;
        // lane (li, g) reads element d = 16 u + 4 e + g of its row for MFMA e: lane group g is the k index of
        // v_mfma_f32_16x16x4_f32, so MFMA e of group u covers d = 16 u + 4 e .. + 3 and the chain runs in rising d
        const float* xa = xl + (16 * rb + li) * pitch + col_off(k) + g;
        for (int bi = 0; bi * UB < ucnt; ++bi) {    // bound: 16 / UB batches
          load_w(fwn, k * (LP_SC / 16 / UB) + bi + 1);
#pragma unroll
          for (int i = 0; i < UB; ++i) {
            const int u = UB * bi + i;
            if (u < ucnt) {
              float fx[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) fx[e] = xa[16 * u + 4 * e];
#pragma unroll
              for (int fi = 0; fi < FC; ++fi)
                if (cb0 + 2 * fi < CB) {
#pragma unroll
                  for (int e = 0; e < 4; ++e) facc[fi] = __builtin_amdgcn_mfma_f32_16x16x4f32(fx[e], fw[i][fi][e], facc[fi], 0, 0, 0);
                }
            }
          }
#pragma unroll
          for (int i = 0; i < UB; ++i)
#pragma unroll
            for (int fi = 0; fi < FC; ++fi) fw[i][fi] = fwn[i][fi];
        }
      }
    }
    // D[row = 4 g + r][col = li]: tile row 16 rb + 4 g + r, class 16 cb + li; z = chain + b
#pragma unroll
    for (int i = 0; i < FC; ++i) {
      const int cb = cb0 + 2 * i;
      if (cb < CB) {
        const int c = 16 * cb + li;
        const float bias = c < C ? a.b[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) zr[(16 * rb + 4 * g + r) * LP_ZP + c] = facc[i][r] + bias;
      }
    }
    __syncthreads();

    // ---- residual pass: 8 lanes a row, lane j takes classes j, j + 8, ...
    const int row = tid >> 3, j8 = tid & 7;
    const int64_t gi = r0 + row;
    const bool valid = gi < a.n;
    float* zrow = zr + row * LP_ZP;
    if (lead && a.logits && valid)
      for (int c = j8; c < C; c += 8) a.logits[gi * C + c] = zrow[c];        // bound: ceil(C / 8)
    if constexpr (!FWD_ONLY) {
      double term = 0.0;
      float wgt = 0.f;
      if (a.loss == SSLCR_LINPROBE_SOFTMAX) {
        const int64_t y = valid ? a.labels[gi] : -1;
        const bool ok = valid && y >= 0 && y < C;
        wgt = ok ? (a.sample_weight ? a.sample_weight[gi] : 1.f) : 0.f;
        const float zy = ok ? zrow[y] : 0.f;
        float m = -INFINITY;
        for (int c = j8; c < C; c += 8) m = fmaxf(m, zrow[c]);              // bound: ceil(C / 8)
        for (int d = 1; d <= 4; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));    // bound: 3 steps
        float e[8], s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = j8 + 8 * k;
          e[k] = c < C ? expf(zrow[c] - m) : 0.f;
          if (c < C) s += e[k];
        }
        for (int d = 1; d <= 4; d <<= 1) s += __shfl_xor(s, d);             // bound: 3 steps of a butterfly: a fixed order
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = j8 + 8 * k;
          if (c < CP) zrow[c] = (ok && c < C) ? (float)((double)wgt * ((double)e[k] / (double)s - (c == y ? 1.0 : 0.0))) : 0.f;
        }
        if (ok) term = (double)wgt * ((double)logf(s) + ((double)m - (double)zy));
      } else {
        wgt = valid ? (a.sample_weight ? a.sample_weight[gi] : 1.f) : 0.f;
        double qs = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = j8 + 8 * k;
          if (c < CP) {
            const bool in = valid && c < C;
            const double diff = in ? (double)zrow[c] - (double)a.targets[gi * C + c] : 0.0;
            qs += diff * diff;
            zrow[c] = in ? (float)((double)wgt * diff) : 0.f;
          }
        }
        for (int d = 1; d <= 4; d <<= 1) qs += __shfl_xor(qs, d);           // bound: 3 steps
        term = (double)wgt * (0.5 * qs);
      }
      if (j8 == 0) { lt[row] = term; lw[row] = (double)wgt; }
      __syncthreads();

      if (lead && wave == 0) {                      // the tile's loss terms: a butterfly over the 32 rows in float64, a fixed order
        double lv = lane < LP_TM ? lt[lane & (LP_TM - 1)] : 0.0, ww = lane < LP_TM ? lw[lane & (LP_TM - 1)] : 0.0;
        for (int d = 32; d >= 1; d >>= 1) { lv += __shfl_xor(lv, d); ww += __shfl_xor(ww, d); }   // bound: 6 steps
        lsum += lv;
        wsum += ww;
      }
      if (lead && wave == 1 && lane < C)
        for (int r = 0; r < LP_TM; ++r) gb += zr[r * LP_ZP + lane];         // bound: 32 rows, rising

      // ---- second product: G += R^T X; A[class][row], B[row][column], 8 row steps of 4 rows, rising
      float af[LP_KS][CB];
#pragma unroll
      for (int ks = 0; ks < LP_KS; ++ks)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) af[ks][cb] = zr[(4 * ks + g) * LP_ZP + 16 * cb + li];
      for (int k = 0; k < (streamed ? nsc : 1); ++k) {                         // bound: the stages again (streamed), or one trip
        if (streamed) {                             // the streamed form fetches the tile again (lines this workgroup has just read)
          commit(k);
          if (k + 1 < nsc) issue(r0, k + 1);
          else if (t + 1 < t_hi) issue(r0 + LP_TM, 0);
          __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int col0 = 16 * (sl * 4 * NB + wave + 4 * j);
          if (col0 < Dp && (!streamed || (col0 >> 8) == k)) {               // wave-uniform: this column block is in LDS now
            const float* xb = xl + g * pitch + col_off(col0 >> 8) + (col0 & (LP_SC - 1)) + li;
#pragma unroll
            for (int ks = 0; ks < LP_KS; ++ks) {
              const float bx = xb[4 * ks * pitch];
#pragma unroll
              for (int cb = 0; cb < CB; ++cb) acc[j][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ks][cb], bx, acc[j][cb], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();                                // every read of the tile and of the residuals before the next tile's stores
  }

  if constexpr (!FWD_ONLY) {
    // D[row = 4 g + r][col = li] of block (j, cb): class 16 cb + 4 g + r, column 16 (s 4 NB + wave + 4 j) + li
    float* pb = part + (int64_t)grp * C * (D + 1);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int d = 16 * (sl * 4 * NB + wave + 4 * j) + li;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cls = 16 * cb + 4 * g + r;
          if (cls < C && d < D) pb[(int64_t)cls * (D + 1) + d] = acc[j][cb][r];
        }
    }
    if (lead && wave == 1 && lane < C) pb[(int64_t)lane * (D + 1) + D] = gb;
    if (lead && tid == 0) { lossp[2 * grp] = lsum; lossp[2 * grp + 1] = wsum; }
  }
}

// ------------------------------------------------------------------------------------------------ 2. fold
// A workgroup folds LP_FE gradient elements: all 256 threads fetch a [64 workgroups][LP_FE elements] tile of the partials into LDS (16
// independent loads a thread), then thread e adds its column in float64 in RISING workgroup order.  Every workgroup sums the loss
// terms and the weights the same way (from LDS, rising), so that all divide by the same total.
constexpr int LP_FE = 64;
__global__ __launch_bounds__(256) void linprobe_fold_kernel(const double* lossp, const float* part, double* value, double* grad, int G, int E) {
  __shared__ float tile[64][LP_FE + 1];
  __shared__ double lp[2 * SSLCR_LINPROBE_MAX_GROUPS];
  __shared__ double tot[2];
  const int tid = threadIdx.x, col = tid & (LP_FE - 1), r4 = tid >> 6;
  for (int i = tid; i < 2 * G; i += 256) lp[i] = lossp[i];                                 // bound: 8 per thread
  __syncthreads();
  if (tid == 0) {
    double l = 0.0, w = 0.0;
    for (int g = 0; g < G; ++g) { l += lp[2 * g]; w += lp[2 * g + 1]; }                    // bound: G workgroups, rising
    tot[0] = l;
    tot[1] = w;
  }
  const int e = blockIdx.x * LP_FE + col;
  double s = 0.0;
  for (int g0 = 0; g0 < G; g0 += 64) {              // bound: ceil(G / 64) tiles
    __syncthreads();                                // the tile before has been summed
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int g = g0 + r4 + 4 * i;
      tile[r4 + 4 * i][col] = (g < G && e < E) ? part[(int64_t)g * E + e] : 0.f;
    }
    __syncthreads();
    if (tid < LP_FE)
      for (int i = 0; i < 64 && g0 + i < G; ++i) s += (double)tile[i][tid];                // bound: 64 workgroups, rising
  }
  __syncthreads();                                  // tot
  if (tid < LP_FE && e < E) grad[e] = s / tot[1];
  if (blockIdx.x == 0 && tid == 0) *value = tot[0] / tot[1];
}

// ------------------------------------------------------------------------------------------------ plan and launch
namespace {
struct LpShape { int CB, NB, S; };
// the accumulator shape of (C, Dp): the smallest NB whose four waves cover the columns in one slice, else the largest a wave holds
LpShape lp_shape(int C, int Dp) {
  const int CB = C <= 16 ? 1 : C <= 32 ? 2 : 4, blocks = Dp / 16, nbmax = 32 / CB;
  int NB = 8;
  while (NB < nbmax && 4 * NB < blocks) NB *= 2;    // bound: 8, 16, 32
  return {CB, NB, (blocks + 4 * NB - 1) / (4 * NB)};
}
size_t lp_align16(size_t v) { return (v + 15) & ~(size_t)15; }
size_t lp_lds_bytes(int cols) { return sizeof(float) * LP_TM * (lp_pitch(cols) + LP_ZP) + sizeof(double) * 2 * LP_TM; }
}  // namespace

const char* linprobe_plan(int n, int D, int C, int loss, int groups_hint, LinprobePlan* out) {
  if (n < 1 || n > 0x7fffffff - 64) return "n outside [1, 2^31 - 64)";
  if (D < 4 || D > SSLCR_LINPROBE_MAX_D || D % 4 != 0) return "D % 4 == 0 and 4 <= D <= 2048";
  if (C < 1 || C > SSLCR_LINPROBE_MAX_C) return "C outside [1, 64]";
  if (loss != SSLCR_LINPROBE_SOFTMAX && loss != SSLCR_LINPROBE_SQUARED) return "loss outside {0, 1}";
  if (groups_hint < 0) return "groups < 0";
  const int Dp = (D + 15) & ~15, tiles = (int)(((int64_t)n + LP_TM - 1) / LP_TM);
  const LpShape sh = lp_shape(C, Dp);
  const bool staged = lp_lds_bytes(Dp) <= LP_STAGED_MAX;
  const int chunk = staged ? Dp : LP_KW;
  const size_t lds = lp_lds_bytes(chunk);
  int G, tpg;
  if (groups_hint > 0) {
    G = groups_hint < tiles ? groups_hint : tiles;
    if (G > SSLCR_LINPROBE_MAX_GROUPS) G = SSLCR_LINPROBE_MAX_GROUPS;
    tpg = (tiles + G - 1) / G;                      // (under a hint a trailing workgroup may own no tile: it writes zero partials)
  } else {
    const int per_cu = LP_LDS_CAP / lds >= 2 ? 2 : 1;   // by LDS alone: the register budget of the NB = 16 / 32 shapes is not measured
    int slots = 256 * per_cu / sh.S;                // workgroups the chip holds at once, shared among the column slices
    if (slots < 1) slots = 1;
    G = tiles < slots ? tiles : slots;
    tpg = (tiles + G - 1) / G;
    G = (tiles + tpg - 1) / tpg;                    // no empty workgroup
  }
  out->form = staged ? SSLCR_LINPROBE_STAGED : SSLCR_LINPROBE_STREAMED;
  out->tile_rows = LP_TM;
  out->groups = G;
  out->tiles_per_group = tpg;
  out->col_slices = sh.S;
  out->chunk = chunk;
  out->class_blocks = sh.CB;
  out->grid[0] = (16 * sh.CB * Dp + 255) / 256;
  out->grid[1] = G * sh.S;
  out->grid[2] = (C * (D + 1) + LP_FE - 1) / LP_FE;
  out->lds_bytes = lds;
  out->workspace_bytes = lp_align16(sizeof(float) * 16 * sh.CB * Dp) + lp_align16(sizeof(double) * 2 * G) +
                         lp_align16(sizeof(float) * (size_t)G * C * (D + 1));
  return nullptr;
}

template <int CB, int NB, bool FWD_ONLY>
static hipError_t lp_launch(const sslcr_linprobe_desc& a, const LinprobePlan& p, const float* wp, double* lossp, float* part, const LpGeom& q,
                            hipStream_t st) {
  return launch_lds<linprobe_kernel<CB, NB, FWD_ONLY>>(dim3((unsigned)p.groups, (unsigned)(FWD_ONLY ? 1 : p.col_slices)), dim3(256), p.lds_bytes,
                                                       LP_LDS_CAP, st, a, wp, lossp, part, q);
}

hipError_t launch_linprobe(const sslcr_linprobe_desc& a, const LinprobePlan& p, bool fwd_only, hipStream_t st) {
  const int Dp = (a.D + 15) & ~15, rows = 16 * p.class_blocks;
  const LpShape sh = lp_shape(a.C, Dp);
  char* ws = static_cast<char*>(a.workspace);
  float* wp = reinterpret_cast<float*>(ws);
  double* lossp = reinterpret_cast<double*>(ws + lp_align16(sizeof(float) * rows * Dp));
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(lossp) + lp_align16(sizeof(double) * 2 * p.groups));
  LpGeom q;
  q.tiles = (int)(((int64_t)a.n + LP_TM - 1) / LP_TM);
  q.tpg = p.tiles_per_group;
  q.Dp = Dp;
  q.streamed = p.form == SSLCR_LINPROBE_STREAMED;
  q.pitch = lp_pitch(p.chunk);
  hipLaunchKernelGGL(linprobe_pack_kernel, dim3((unsigned)p.grid[0]), dim3(256), 0, st, a.w, wp, a.C, a.D, Dp, rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (fwd_only) {
    e = sh.CB == 1 ? lp_launch<1, 1, true>(a, p, wp, lossp, part, q, st)
      : sh.CB == 2 ? lp_launch<2, 1, true>(a, p, wp, lossp, part, q, st) : lp_launch<4, 1, true>(a, p, wp, lossp, part, q, st);
    return e;
  }
  if (sh.CB == 1) e = sh.NB == 8 ? lp_launch<1, 8, false>(a, p, wp, lossp, part, q, st)
                    : sh.NB == 16 ? lp_launch<1, 16, false>(a, p, wp, lossp, part, q, st) : lp_launch<1, 32, false>(a, p, wp, lossp, part, q, st);
  else if (sh.CB == 2) e = sh.NB == 8 ? lp_launch<2, 8, false>(a, p, wp, lossp, part, q, st) : lp_launch<2, 16, false>(a, p, wp, lossp, part, q, st);
  else e = lp_launch<4, 8, false>(a, p, wp, lossp, part, q, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(linprobe_fold_kernel, dim3((unsigned)p.grid[2]), dim3(256), 0, st, lossp, part, a.value, a.grad, p.groups, a.C * (a.D + 1));
  return hipGetLastError();
}

}  // namespace sslcr
