// Camelyon16 lesion scoring on the device: from a probability map and a truth mask to what lesion-level FROC counts.  Four pieces
// (include/sslcr.h has the contracts and the definitions):
//   label_components  connected components of the truth mask, numbered 1..L by the order of each component's first cell
//   gaussian_smooth   the optional separable float32 Gaussian of the map, edge mode "nearest", axis 0 then axis 1
//   nms_*             greedy non-maximum suppression of the map into a detection list: candidates, rounds, collect
//   lesion_hits       the label under every detection, the best probability per lesion, the lesions' areas
// Built with -ffp-contract=off: a smoothing tap is one float32 product and one float32 sum, each rounded on its own.
// Every atomic here is an integer min, max or add: the results do not depend on the order in which they land.  Work proceeds
// between workgroups through launch boundaries only; no kernel waits for another workgroup, and every loop states its bound.
#include "kernels.hpp"
#include "map_common.hpp"

namespace sslcr {

// ------------------------------------------------------------------------------------------------ 1. connected components
// Union-find over linear indices g = x * Y + y.  parent[g] < 0 for a zero cell; otherwise parent[g] <= g always, so a walk to the root
// strictly descends and ends after at most g steps, and a root is the lowest index its tree has seen.  A union links the HIGHER root
// under the lower one with an atomicMin: whatever the order of the unions, the root of a finished component is its lowest index.
//   cc_local     a workgroup owns a CC_TX x CC_TY tile: mask bytes fetched as whole dwords of the flat array, unions of every cell with
//                its W / N (and NW / NE) neighbour inside the tile in LDS, then every cell's parent = the tile-local root, as a linear index
//   cc_borders   one thread per cell of a tile's first row / first column: unions with the cells across the border -- for
//                connectivity 2 the diagonal ones too, which covers the neighbours across tile corners
//   cc_flatten   parent[g] = root, and the number of roots of every run of CC_SCAN cells
//   cc_offsets   one workgroup: exclusive scan of those counts in run order (= row-major order), and L
//   cc_number    the roots get their number (stored as -(number) - 1 in parent), then cc_relabel writes labels
constexpr int CC_TX = 16, CC_TY = 64, CC_CELLS = CC_TX * CC_TY, CC_SCAN = SSLCR_LABEL_RUN_CELLS;
static_assert(CC_SCAN == 4 * 256, "a run is one workgroup's cells, four per thread");
constexpr int CC_ROW_DWORDS = CC_TY / 4 + 1;     // aligned dwords that cover CC_TY bytes starting anywhere

__device__ __forceinline__ int cc_find(const int* parent, int i) {
  const int bound = i;
  for (int k = 0; k <= bound; ++k) {              // bound: the walk strictly descends from where it starts
    const int p = parent[i];
    if (p == i) break;
    i = p;
  }
  return i;
}

__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  const int bound = a > b ? a : b;
  for (int k = 0; k <= bound; ++k) {              // bound: every retry continues from a strictly lower index
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;                         // a was a root and now hangs under b
    a = old;                                      // somebody linked a first: go on from where it points
  }
}

__global__ __launch_bounds__(256) void cc_local_kernel(const sslcr_label_desc a, int tiles_y) {
  __shared__ unsigned char m[CC_TX][CC_TY];
  __shared__ int par[CC_CELLS];
  const int t = threadIdx.x;
  const int x0 = (int)(blockIdx.x / tiles_y) * CC_TX, y0 = (int)(blockIdx.x % tiles_y) * CC_TY;
  const int nxr = min(CC_TX, a.X - x0), nyr = min(CC_TY, a.Y - y0);
  const int64_t n = (int64_t)a.X * a.Y;
  for (int i = t; i < CC_CELLS; i += 256) m[i / CC_TY][i % CC_TY] = 0;
  __syncthreads();
  for (int i = t; i < CC_TX * CC_ROW_DWORDS; i += 256) {
    const int r = i / CC_ROW_DWORDS, k = i % CC_ROW_DWORDS;
    if (r >= nxr) continue;
    const int64_t start = (int64_t)(x0 + r) * a.Y + y0, addr = (start & ~(int64_t)3) + 4 * k;
    if (addr >= start + nyr) continue;
    const unsigned v = mask_dword(a.mask, addr, n);
    for (int j = 0; j < 4; ++j) {
      const int64_t c = addr + j - start;
      if (c >= 0 && c < nyr) m[r][c] = (unsigned char)((v >> (8 * j)) & 0xffu);
    }
  }
  __syncthreads();
  for (int i = t; i < CC_CELLS; i += 256) par[i] = m[i / CC_TY][i % CC_TY] ? i : -1;
  __syncthreads();
  const bool diag = a.connectivity == 2;
  for (int i = t; i < CC_CELLS; i += 256) {
    const int r = i / CC_TY, c = i % CC_TY;
    if (!m[r][c]) continue;
    if (c > 0 && m[r][c - 1]) cc_union(par, i, i - 1);
    if (r > 0) {
      if (m[r - 1][c]) cc_union(par, i, i - CC_TY);
      if (diag && c > 0 && m[r - 1][c - 1]) cc_union(par, i, i - CC_TY - 1);
      if (diag && c + 1 < CC_TY && m[r - 1][c + 1]) cc_union(par, i, i - CC_TY + 1);
    }
  }
  __syncthreads();
  for (int i = t; i < CC_CELLS; i += 256) {
    const int r = i / CC_TY, c = i % CC_TY;
    if (r >= nxr || c >= nyr) continue;
    int v = -1;
    if (m[r][c]) {
      const int root = cc_find(par, i);
      v = (x0 + root / CC_TY) * a.Y + y0 + root % CC_TY;
    }
    a.work[(int64_t)(x0 + r) * a.Y + y0 + c] = v;
  }
}

// thread i < rows * Y: cell (CC_TX * (1 + i / Y), i % Y) against the row above; the others: cell (x, CC_TY * (1 + k)) against the
// column to its left.  The diagonal pairs across a tile corner are met from one side or the other (some from both: a union twice is one).
__global__ __launch_bounds__(256) void cc_borders_kernel(const sslcr_label_desc a, int64_t row_cells, int64_t col_cells, int cols) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int* parent = a.work;
  const bool diag = a.connectivity == 2;
  if (i < row_cells) {
    const int x = CC_TX * (1 + (int)(i / a.Y)), y = (int)(i % a.Y);
    const int g = x * a.Y + y;
    if (parent[g] < 0) return;
    if (parent[g - a.Y] >= 0) cc_union(parent, g, g - a.Y);
    if (diag && y > 0 && parent[g - a.Y - 1] >= 0) cc_union(parent, g, g - a.Y - 1);
    if (diag && y + 1 < a.Y && parent[g - a.Y + 1] >= 0) cc_union(parent, g, g - a.Y + 1);
  } else if (i < row_cells + col_cells) {
    const int64_t j = i - row_cells;
    const int x = (int)(j / cols), y = CC_TY * (1 + (int)(j % cols));
    const int g = x * a.Y + y;
    if (parent[g] < 0) return;
    if (parent[g - 1] >= 0) cc_union(parent, g, g - 1);
    if (diag && x > 0 && parent[g - a.Y - 1] >= 0) cc_union(parent, g, g - a.Y - 1);
    if (diag && x + 1 < a.X && parent[g + a.Y - 1] >= 0) cc_union(parent, g, g + a.Y - 1);
  }
}

// thread t of run b holds the cells b * CC_SCAN + 4 t .. + 3; all 256 threads of the three kernels below reach block_excl_sum
__global__ __launch_bounds__(256) void cc_flatten_kernel(const sslcr_label_desc a, int* run_roots) {
  __shared__ int sh[4];
  const int64_t n = (int64_t)a.X * a.Y, base = (int64_t)blockIdx.x * CC_SCAN + 4 * threadIdx.x;
  int roots = 0;
  for (int j = 0; j < 4; ++j) {
    const int64_t g = base + j;
    if (g >= n || a.work[g] < 0) continue;
    const int r = cc_find(a.work, (int)g);
    if (r == (int)g) ++roots;
    else a.work[g] = r;                           // a root keeps itself; any value a concurrent walk reads here is an ancestor
  }
  int total;
  block_excl_sum(roots, sh, &total);
  if (threadIdx.x == 0) run_roots[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void cc_offsets_kernel(int* run_roots, int runs, int* count) {
  __shared__ int sh[4];
  int carry = 0;
  for (int base = 0; base < runs; base += 256) {  // bound: runs / 256 rounds
    const int i = base + threadIdx.x;
    const int v = i < runs ? run_roots[i] : 0;
    int total;
    const int ex = block_excl_sum(v, sh, &total);
    if (i < runs) run_roots[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(256) void cc_number_kernel(const sslcr_label_desc a, const int* run_offsets) {
  __shared__ int sh[4];
  const int64_t n = (int64_t)a.X * a.Y, base = (int64_t)blockIdx.x * CC_SCAN + 4 * threadIdx.x;
  bool root[4];
  int mine = 0;
  for (int j = 0; j < 4; ++j) {
    const int64_t g = base + j;
    root[j] = g < n && a.work[g] == (int)g;
    mine += root[j];
  }
  int total;
  int number = run_offsets[blockIdx.x] + block_excl_sum(mine, sh, &total);
  for (int j = 0; j < 4; ++j)
    if (root[j]) a.work[base + j] = -(++number) - 1;      // <= -2: a numbered root; -1 stays the zero cell
}

__global__ __launch_bounds__(256) void cc_relabel_kernel(const sslcr_label_desc a) {
  const int64_t n = (int64_t)a.X * a.Y, g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const int v = a.work[g];
  a.labels[g] = v == -1 ? 0 : v <= -2 ? -v - 1 : -a.work[v] - 1;
}

hipError_t launch_label_components(const sslcr_label_desc& a, hipStream_t st) {
  const int64_t n = (int64_t)a.X * a.Y;
  const int tiles_x = (a.X + CC_TX - 1) / CC_TX, tiles_y = (a.Y + CC_TY - 1) / CC_TY;
  const int runs = (int)((n + CC_SCAN - 1) / CC_SCAN);
  int* run_roots = a.work + n;                                               // work: [n] parents, then [runs] counts / offsets
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(256), 0, st, a, tiles_y);
  const int64_t row_cells = (int64_t)((a.X - 1) / CC_TX) * a.Y;
  const int cols = (a.Y - 1) / CC_TY;
  const int64_t col_cells = (int64_t)cols * a.X;
  if (row_cells + col_cells > 0)
    hipLaunchKernelGGL(cc_borders_kernel, dim3((unsigned)((row_cells + col_cells + 255) / 256)), dim3(256), 0, st, a, row_cells, col_cells, cols);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)runs), dim3(256), 0, st, a, run_roots);
  hipLaunchKernelGGL(cc_offsets_kernel, dim3(1), dim3(256), 0, st, run_roots, runs, a.count);
  hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)runs), dim3(256), 0, st, a, (const int*)run_roots);
  hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. Gaussian smoothing
// One thread per cell and pass: acc = 0; for k = -R .. R: acc = acc + w[k + R] * src[clamp(i + k)], a float32 product then a float32
// sum (no contraction in this translation unit).  Axis 0 from src into tmp, axis 1 from tmp into dst.
__global__ __launch_bounds__(256) void gauss_pass_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                         const float* __restrict__ w, int X, int Y, int R, int axis) {
  const int64_t n = (int64_t)X * Y, g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const int x = (int)(g / Y), y = (int)(g % Y);
  float acc = 0.f;
  for (int k = -R; k <= R; ++k) {                  // bound: 2 R + 1 <= 129 taps
    float v;
    if (axis == 0) v = src[(int64_t)min(max(x + k, 0), X - 1) * Y + y];
    else v = src[(int64_t)x * Y + min(max(y + k, 0), Y - 1)];
    const float p = w[k + R] * v;
    acc = acc + p;
  }
  dst[g] = acc;
}

hipError_t launch_gaussian_smooth(const sslcr_smooth_desc& a, hipStream_t st) {
  const int64_t n = (int64_t)a.X * a.Y;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(gauss_pass_kernel, dim3(blocks), dim3(256), 0, st, a.src, a.tmp, a.weights, a.X, a.Y, a.R, 0);
  hipLaunchKernelGGL(gauss_pass_kernel, dim3(blocks), dim3(256), 0, st, (const float*)a.tmp, a.dst, a.weights, a.X, a.Y, a.R, 1);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 3. non-maximum suppression
// state[X][Y], one byte per cell: 0 no candidate, 1 undecided, 2 selected, 3 suppressed.  A decision, once stored, is final and is
// the definition's; a round decides a candidate from the states it READS: a selected predecessor whose window holds it suppresses it,
// an undecided one leaves it undecided, neither selects it.  A byte another thread of the same launch is storing reads as 1 or as its
// final value: both are sound, so the rounds need nothing from one another but the launch boundary.
//   counters[0] candidates   counters[1] undecided after the last counted round   counters[2] selected   counters[3] spare
constexpr unsigned char NMS_NONE = 0, NMS_UNDECIDED = 1, NMS_SELECTED = 2, NMS_SUPPRESSED = 3;

__global__ __launch_bounds__(256) void nms_candidates_kernel(const sslcr_nms_desc a) {
  const int64_t n = (int64_t)a.X * a.Y, g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool cand = g < n && a.map[g] > a.threshold;                         // a NaN compares false
  if (g < n) a.state[g] = cand ? NMS_UNDECIDED : NMS_NONE;
  const unsigned long long votes = __ballot(cand);                           // wave_vote_add's add, and a slot for every voting lane
  if (!votes) return;
  const int lane = threadIdx.x & 63, leader = __ffsll(votes) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(&a.counters[0], __popcll(votes));
  base = __shfl(base, leader);
  if (cand) a.cand[base + __popcll(votes & ((1ull << lane) - 1ull))] = (int)g;    // at most n candidates, cand holds n
}

// bytes of v equal to zero -> their high bits (it may also flag a byte above a zero byte: a quick reject, never a verdict)
__device__ __forceinline__ unsigned zero_bytes(unsigned v) { return (v - 0x01010101u) & ~v & 0x80808080u; }

// The window's states are read as aligned dwords of the flat array, four cells at a time; a dword without a selected byte -- and, until
// the first undecided predecessor is found, without an undecided one -- costs nothing more.  On a plateau below the front of decisions
// every cell is undecided: the scan then reads one map value and (2 r)^2 / 4 dwords, not (2 r)^2 bytes and values.
__global__ __launch_bounds__(256) void nms_round_kernel(const sslcr_nms_desc a, int count_left) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t n = (int64_t)a.X * a.Y;
  bool left = false;
  if (i < a.ncand) {
    const int p = a.cand[i];
    if (a.state[p] == NMS_UNDECIDED) {
      const int px = p / a.Y, py = p % a.Y;
      const float vp = a.map[p];
      // p lies in q's window [qx - r, qx + r) x [qy - r, qy + r)  <=>  qx in [px - r + 1, px + r], qy alike
      const int64_t lx = (int64_t)px - a.radius + 1, hx = (int64_t)px + a.radius, ly = (int64_t)py - a.radius + 1, hy = (int64_t)py + a.radius;
      const int qx0 = lx < 0 ? 0 : (int)lx, qx1 = hx > a.X - 1 ? a.X - 1 : (int)hx;
      const int qy0 = ly < 0 ? 0 : (int)ly, qy1 = hy > a.Y - 1 ? a.Y - 1 : (int)hy;
      bool suppressed = false, waits = false;
      for (int qx = qx0; qx <= qx1 && !suppressed; ++qx) {                   // bound: at most (2 r)^2 cells, clipped to the map
        const int64_t lo = (int64_t)qx * a.Y + qy0, hi = (int64_t)qx * a.Y + qy1;
        for (int64_t w = lo & ~(int64_t)3; w <= hi && !suppressed; w += 4) {
          const unsigned v = mask_dword(a.state, w, n);
          if (!(zero_bytes(v ^ 0x02020202u) | (waits ? 0u : zero_bytes(v ^ 0x01010101u)))) continue;
          for (int j = 0; j < 4; ++j) {
            const int64_t q = w + j;
            const unsigned s = (v >> (8 * j)) & 0xffu;
            if (q < lo || q > hi || q == p || !(s == NMS_SELECTED || (s == NMS_UNDECIDED && !waits))) continue;
            const float vq = a.map[q];
            if (!(vq > vp || (vq == vp && q < p))) continue;                 // q does not precede p
            if (s == NMS_SELECTED) {
              suppressed = true;
              break;
            }
            waits = true;
          }
        }
      }
      if (suppressed) a.state[p] = NMS_SUPPRESSED;
      else if (!waits) a.state[p] = NMS_SELECTED;
      else left = true;
    }
  }
  if (count_left) wave_vote_add(&a.counters[1], left);
}

// the selected candidates, in any order, into the staging list (the upper half of det_xy / det_prob's workspace `stage`)
__global__ __launch_bounds__(256) void nms_gather_kernel(const sslcr_nms_desc a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.ncand) return;
  const int p = a.cand[i];
  if (a.state[p] != NMS_SELECTED) return;
  const int slot = atomicAdd(&a.counters[2], 1);
  if (slot < a.max_detections) a.stage[slot] = p;                            // past the capacity: counted, not stored
}

// output order is "precedes" order: a detection's place is the number of detections that precede it (a strict total order)
__global__ __launch_bounds__(256) void nms_order_kernel(const sslcr_nms_desc a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = min(a.counters[2], a.max_detections);
  if (i >= k) return;
  const int p = a.stage[i];
  const float vp = a.map[p];
  int rank = 0;
  for (int j = 0; j < k; ++j) {                                              // bound: k <= max_detections
    const int q = a.stage[j];
    const float vq = a.map[q];
    rank += (vq > vp || (vq == vp && q < p)) ? 1 : 0;
  }
  a.det_xy[2 * rank] = p / a.Y;
  a.det_xy[2 * rank + 1] = p % a.Y;
  a.det_prob[rank] = vp;
}

hipError_t launch_nms_candidates(const sslcr_nms_desc& a, hipStream_t st) {
  const int64_t n = (int64_t)a.X * a.Y;
  hipError_t e = hipMemsetAsync(a.counters, 0, 4 * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nms_candidates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_nms_rounds(const sslcr_nms_desc& a, int rounds, hipStream_t st) {
  if (a.ncand == 0 || rounds == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.counters + 1, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((a.ncand + 255) / 256);
  for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(nms_round_kernel, dim3(blocks), dim3(256), 0, st, a, r == rounds - 1 ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_nms_collect(const sslcr_nms_desc& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.counters + 2, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  if (a.ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(nms_gather_kernel, dim3((unsigned)((a.ncand + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(nms_order_kernel, dim3((unsigned)((a.max_detections + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 4. hits and areas
// The first workgroups take the detections: hit = the label under it; a hit on a lesion that is not ignored raises that lesion's
// best probability -- an integer atomicMax on the float's bits, which orders non-negative floats as the floats (a probability that is
// not above +0 cannot raise the initial 0 and is left out).  In the other workgroups a wave takes AREA_STEPS runs of 64 consecutive
// cells; per run it counts each distinct label with ballots and keeps the count of the label it met last in (wave-uniform) registers,
// so a stretch of one lesion costs one int64 atomic per wave and not one per cell: the large lesions are where the adds would pile up.
constexpr int AREA_STEPS = 16;

__global__ __launch_bounds__(256) void lesion_hits_kernel(const sslcr_hits_desc a, int det_blocks) {
  if ((int)blockIdx.x < det_blocks) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int ndet = min(*a.n_det, a.max_detections);
    if (k >= ndet) return;
    const int x = a.det_xy[2 * k], y = a.det_xy[2 * k + 1];
    int label = 0;
    if (x >= 0 && x < a.X && y >= 0 && y < a.Y) label = a.labels[(int64_t)x * a.Y + y];
    a.hit[k] = label;
    if (label < 1 || label > a.L) return;
    for (int j = 0; j < a.n_ignore; ++j)                                     // bound: n_ignore
      if (a.ignore[j] == label) return;
    const float p = a.det_prob[k];
    if (p > 0.f) atomicMax(reinterpret_cast<int*>(a.tp_prob) + (label - 1), __float_as_int(p));
    return;
  }
  if (!a.areas) return;
  const int64_t n = (int64_t)a.X * a.Y;
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)(blockIdx.x - det_blocks) * 4 + (threadIdx.x >> 6)) * (64 * AREA_STEPS);
  unsigned long long* areas = reinterpret_cast<unsigned long long*>(a.areas);
  int current = 0;                                                           // wave-uniform, like run
  unsigned long long run = 0;
  for (int j = 0; j < AREA_STEPS; ++j) {
    const int64_t g = base + 64 * j + lane;
    int label = g < n ? a.labels[g] : 0;
    if (label < 1 || label > a.L) label = 0;
    unsigned long long todo = __ballot(label != 0);                          // (region_moments_kernel, evalmask.hip, walks its labels alike)
    for (int k = 0; k < 64 && todo; ++k) {                                   // bound: 64 lanes hold at most 64 distinct labels
      const int which = __shfl(label, __ffsll(todo) - 1);
      const unsigned long long same = __ballot(label == which);
      if (which != current) {
        if (current && lane == 0) atomicAdd(areas + (current - 1), run);
        current = which;
        run = 0;
      }
      run += (unsigned long long)__popcll(same);
      todo &= ~same;
    }
  }
  if (current && lane == 0) atomicAdd(areas + (current - 1), run);
}

hipError_t launch_lesion_hits(const sslcr_hits_desc& a, hipStream_t st) {
  const int64_t n = (int64_t)a.X * a.Y;
  const int det_blocks = (a.max_detections + 255) / 256;
  const int64_t area_blocks = a.areas ? (n + 256 * AREA_STEPS - 1) / (256 * AREA_STEPS) : 0;
  if (det_blocks + area_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(lesion_hits_kernel, dim3((unsigned)(det_blocks + area_blocks)), dim3(256), 0, st, a, det_blocks);
  return hipGetLastError();
}

}  // namespace sslcr
