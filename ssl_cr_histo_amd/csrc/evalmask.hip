// The Camelyon16 evaluation mask on the device: what the challenge's computeEvaluationMask / computeITCList take from scipy and
// scikit-image, as integer kernels (include/sslcr.h has the contracts and the definitions):
//   edt_squared     the exact squared Euclidean distance of every cell to the nearest zero cell, capped at a limit
//   fill_holes      the mask plus the background components (connectivity 1) that touch no border cell
//   region_moments  area, sum x, sum y, sum x^2, sum y^2, sum x y of every labelled component, int64
// Integer arithmetic only: there is no floating-point operation in this translation unit.  Every atomic is an integer add, and the
// border pass stores the constant 1: no result depends on the order in which they land.  Work proceeds between workgroups through
// launch boundaries only; no kernel waits for another workgroup, and every loop states its bound.
#include "kernels.hpp"
#include "map_common.hpp"

namespace sslcr {

// ------------------------------------------------------------------------------------------------ 1. squared distance transform
// Two passes (the separable form: min over x' of g(x', y)^2 + (x - x')^2, g = the distance to the nearest zero WITHIN a row).
//   edt_rows     one workgroup per row x: g[x][y] = |y - y'| to the nearest zero cell (x, y') of the row, EDT_NONE where the row has none.
//                The row is walked in chunks of EDT_ROW_CELLS cells, one aligned dword of the flat mask per thread (the staging limit
//                the tests cross): a forward sweep with a prefix max-scan of "the last zero at or before y" (carried from chunk to chunk)
//                stores the distance to the left, a backward sweep with a suffix min-scan of "the first zero at or after y" takes the
//                minimum with the distance to the right.  A thread reads back only what it stored itself.
//   edt_columns  one thread per cell, lanes along y: best = g[x][y]^2, then x' = x -+ d for d = 1, 2, ...; the search ends at
//                d^2 >= best, which is exact: every cell further away in x alone is at least that far.  best starts capped at the
//                limit, so a limited transform walks sqrt(limit) rows at most.
// X^2 + Y^2 < 2^31 (checked at the C-ABI): every g^2 + d^2 formed here fits an int32.
constexpr int EDT_ROW_CELLS = SSLCR_EDT_ROW_CELLS, EDT_NONE = 0x7fffffff;
constexpr int EDT_FAR = 1 << 30;                    // "no zero seen": |EDT_FAR| + a coordinate stays inside an int32
static_assert(EDT_ROW_CELLS == 4 * 256, "one dword per thread and chunk");

__global__ __launch_bounds__(256) void edt_rows_kernel(const sslcr_edt_desc a) {
  __shared__ int sh[4];
  const int t = threadIdx.x, x = blockIdx.x;
  const int64_t n = (int64_t)a.X * a.Y, start = (int64_t)x * a.Y, base = start & ~(int64_t)3;
  const int lead = (int)(start - base);             // cells of the previous row in the first dword
  const int chunks = (lead + a.Y + EDT_ROW_CELLS - 1) / EDT_ROW_CELLS;
  const bool zero_is_set = a.invert != 0;
  int carry = -EDT_FAR;                             // the last zero's y in the chunks already swept
  for (int c = 0; c < chunks; ++c) {                // bound: chunks = ceil((lead + Y) / EDT_ROW_CELLS)
    const int y0 = c * EDT_ROW_CELLS + 4 * t - lead;                         // the row coordinate of this thread's first byte
    const int64_t addr = base + (int64_t)c * EDT_ROW_CELLS + 4 * t;
    const unsigned v = y0 < a.Y ? mask_dword(a.mask, addr, n) : 0u;
    int last = -EDT_FAR;
    bool zero[4];
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + j;
      zero[j] = y >= 0 && y < a.Y && ((((v >> (8 * j)) & 0xffu) != 0) == zero_is_set);
      if (zero[j]) last = y;
    }
    int total;
    const int before = block_scan_max(last, false, -EDT_FAR, sh, &total);     // the threads before this one ...
    int seen = max(before, carry);                                           // ... and the chunks before this one
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + j;
      if (zero[j]) seen = y;
      if (y >= 0 && y < a.Y) a.work[start + y] = seen == -EDT_FAR ? EDT_NONE : y - seen;
    }
    carry = max(carry, total);
  }
  carry = -EDT_FAR;                                 // minus the first zero's y in the chunks already swept, from the right
  for (int c = chunks - 1; c >= 0; --c) {           // bound: chunks
    const int y0 = c * EDT_ROW_CELLS + 4 * t - lead;
    const int64_t addr = base + (int64_t)c * EDT_ROW_CELLS + 4 * t;
    const unsigned v = y0 < a.Y ? mask_dword(a.mask, addr, n) : 0u;
    int first = -EDT_FAR;
    bool zero[4];
    for (int j = 3; j >= 0; --j) {
      const int y = y0 + j;
      zero[j] = y >= 0 && y < a.Y && ((((v >> (8 * j)) & 0xffu) != 0) == zero_is_set);
      if (zero[j]) first = -y;
    }
    int total;
    const int after = block_scan_max(first, true, -EDT_FAR, sh, &total);
    int seen = max(after, carry);
    for (int j = 3; j >= 0; --j) {
      const int y = y0 + j;
      if (zero[j]) seen = -y;
      if (y >= 0 && y < a.Y && seen != -EDT_FAR) {
        const int right = -seen - y, left = a.work[start + y];               // left: stored by this thread in the forward sweep
        if (right < left) a.work[start + y] = right;
      }
    }
    carry = max(carry, total);
  }
}

constexpr int EDT_TY = 64, EDT_TX = 4;              // a workgroup's cells: 4 rows of 64 consecutive y, one wave per row

__global__ __launch_bounds__(256) void edt_columns_kernel(const sslcr_edt_desc a, int tiles_y) {
  const int x = (int)(blockIdx.x / tiles_y) * EDT_TX + (threadIdx.x >> 6), y = (int)(blockIdx.x % tiles_y) * EDT_TY + (threadIdx.x & 63);
  if (x >= a.X || y >= a.Y) return;
  const int* g = a.work;
  const int64_t at = (int64_t)x * a.Y + y;
  const int g0 = g[at];
  int best = g0 == EDT_NONE ? 0x7fffffff : g0 * g0;
  best = min(best, a.limit);
  for (int d = 1; d < a.X; ++d) {                   // bound: X - 1 rows either way
    const int dd = d * d;
    if (dd >= best) break;                          // exact: every row further out is at least d away
    const bool up = x - d >= 0, down = x + d < a.X;
    if (!up && !down) break;
    if (up) {
      const int gv = g[at - (int64_t)d * a.Y];
      if (gv != EDT_NONE) best = min(best, gv * gv + dd);
    }
    if (down) {
      const int gv = g[at + (int64_t)d * a.Y];
      if (gv != EDT_NONE) best = min(best, gv * gv + dd);
    }
  }
  a.out[at] = best;
  if (a.below) a.below[at] = best < a.limit ? 1 : 0;
}

hipError_t launch_edt_squared(const sslcr_edt_desc& a, hipStream_t st) {
  const int tiles_x = (a.X + EDT_TX - 1) / EDT_TX, tiles_y = (a.Y + EDT_TY - 1) / EDT_TY;
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)a.X), dim3(256), 0, st, a);
  hipLaunchKernelGGL(edt_columns_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(256), 0, st, a, tiles_y);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. hole filling
// out doubles as the complement: out = (mask == 0), labelled at connectivity 1 by launch_label_components (froc.hip); the labeller's
// parent array is free once the labels are written and becomes the per-label "reaches the border" flags (zeroed, then plain stores of
// 1 from the border cells); the apply pass then overwrites out with the answer.
__global__ __launch_bounds__(256) void fill_complement_kernel(const sslcr_fill_desc a) {
  const int64_t n = (int64_t)a.X * a.Y, g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < n) a.out[g] = a.mask[g] == 0 ? 1 : 0;
}

// thread i: the cells of row 0, of row X - 1, of column 0, of column Y - 1, in that order (a corner twice: the same store twice)
__global__ __launch_bounds__(256) void fill_border_kernel(const sslcr_fill_desc a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int x, y;
  if (i < a.Y) x = 0, y = (int)i;
  else if (i < 2 * (int64_t)a.Y) x = a.X - 1, y = (int)(i - a.Y);
  else if (i < 2 * (int64_t)a.Y + a.X) x = (int)(i - 2 * (int64_t)a.Y), y = 0;
  else if (i < 2 * ((int64_t)a.Y + a.X)) x = (int)(i - 2 * (int64_t)a.Y - a.X), y = a.Y - 1;
  else return;
  const int label = a.labels[(int64_t)x * a.Y + y];
  if (label > 0) a.work[label - 1] = 1;             // at most ceil(X * Y / 2) components at connectivity 1: inside work's first X * Y
}

__global__ __launch_bounds__(256) void fill_apply_kernel(const sslcr_fill_desc a) {
  const int64_t n = (int64_t)a.X * a.Y, g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const int label = a.labels[g];                    // 0 on a set cell: the complement was labelled
  a.out[g] = (label == 0 || a.work[label - 1] == 0) ? 1 : 0;
}

hipError_t launch_fill_holes(const sslcr_fill_desc& a, hipStream_t st) {
  const int64_t n = (int64_t)a.X * a.Y;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(fill_complement_kernel, dim3(blocks), dim3(256), 0, st, a);
  sslcr_label_desc l;
  l.mask = a.out;
  l.labels = a.labels;
  l.count = a.count;
  l.work = a.work;
  l.X = a.X;
  l.Y = a.Y;
  l.connectivity = 1;
  hipError_t e = launch_label_components(l, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.work, 0, (size_t)n * sizeof(int), st);
  if (e != hipSuccess) return e;
  const int64_t border = 2 * ((int64_t)a.X + a.Y);
  hipLaunchKernelGGL(fill_border_kernel, dim3((unsigned)((border + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(fill_apply_kernel, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 3. region moments
// A wave takes MOM_STEPS runs of 64 consecutive cells (linear index x * Y + y), as lesion_hits does for the areas: per run it takes
// each distinct label with ballots, sums the label's lanes with a butterfly and keeps the sums of the label it met last in
// registers (lane q holds moment q), so a stretch of one component costs six int64 atomics per wave and not six per cell.
// Bounds: X^2 + Y^2 < 2^31 gives x, y < 46341 and x^2, y^2, x y < 2^31; a component has fewer than 2^31 cells: every sum < 2^62.
constexpr int MOM_STEPS = 16;

__global__ __launch_bounds__(256) void region_moments_kernel(const sslcr_moments_desc a) {
  const int64_t n = (int64_t)a.X * a.Y;
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * MOM_STEPS);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(a.moments);
  int current = 0;                                                           // wave-uniform
  unsigned long long acc = 0;                                                // lane q < 6: moment q of the current label
  for (int j = 0; j < MOM_STEPS; ++j) {
    const int64_t g = base + 64 * j + lane;
    int label = g < n ? a.labels[g] : 0;
    if (label < 1 || label > a.L) label = 0;
    const unsigned long long x = g < n ? (unsigned long long)(g / a.Y) : 0, y = g < n ? (unsigned long long)(g % a.Y) : 0;
    // lesion_hits_kernel's walk over the labels (froc.hip); both keep it inline: a shared helper changes the code of both kernels
    unsigned long long todo = __ballot(label != 0);
    for (int k = 0; k < 64 && todo; ++k) {                                   // bound: 64 lanes hold at most 64 distinct labels
      const int which = __shfl(label, __ffsll(todo) - 1);
      const bool mine = label == which;
      const unsigned long long same = __ballot(mine);
      if (which != current) {
        if (current && lane < 6) atomicAdd(out + 6 * (int64_t)(current - 1) + lane, acc);
        current = which;
        acc = 0;
      }
      const unsigned long long mx = mine ? x : 0, my = mine ? y : 0;
      const unsigned long long s[6] = {(unsigned long long)__popcll(same), wave_sum(mx), wave_sum(my), wave_sum(mx * mx), wave_sum(my * my),
                                       wave_sum(mx * my)};
      for (int q = 0; q < 6; ++q)
        if (lane == q) acc += s[q];
      todo &= ~same;
    }
  }
  if (current && lane < 6) atomicAdd(out + 6 * (int64_t)(current - 1) + lane, acc);
}

hipError_t launch_region_moments(const sslcr_moments_desc& a, hipStream_t st) {
  if (a.L == 0) return hipSuccess;
  const int64_t n = (int64_t)a.X * a.Y;
  hipLaunchKernelGGL(region_moments_kernel, dim3((unsigned)((n + 256 * MOM_STEPS - 1) / (256 * MOM_STEPS))), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sslcr
