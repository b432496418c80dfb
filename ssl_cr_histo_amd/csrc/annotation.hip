// Camelyon16 annotations on the device: what Annotation.inside_polygons (util.py:197-205, 246-266) decides per sample on the host --
// the label of a patch (dataset.py:740-743) and the truth a probability map is scored against (dataset.py:985-988) -- for a batch of
// points or for a whole mask grid, and the thresholded confusion counts of a finished map.  Two entries (include/sslcr.h has the
// contracts):
//   points_in_polygons  the crossing-number test of skimage 0.15 points_in_poly for every (point, polygon) pair, any-hit and first-hit
//   map_confusion       confusion[t][truth][p >= thr[t]] over the tissue cells of a map, for up to 64 thresholds in one pass
// Built with -ffp-contract=off: the float64 chain is one subtraction each, one product, one correctly rounded division and one
// addition, in that order; a contracted multiply-add would round once where the definition rounds twice.
// No floating-point atomics.  The point kernel has no atomics at all; the confusion kernel counts in integers.
#include "kernels.hpp"
#include "softmax_row.hpp"   // confusion_flush_cell

namespace sslcr {

// ------------------------------------------------------------------------------------------------ 1. points in polygons
// One lane per point, 256 points per workgroup: a 16 x 16 block of grid cells (each wave an 8 x 8 block, so that a polygon's bounds
// miss a whole wave as often as they can), or 256 consecutive points of the explicit list.
//
// The vertex list is walked ONCE, in chunks of SSLCR_PIP_CHUNK vertices (= edges: edge v ends in vertex v and starts in its polygon's
// previous vertex), whatever the polygons' sizes: a polygon may span chunks, a chunk may span polygons.  Per chunk
//   1. every lane votes whether it still needs one of the chunk's polygons (not decided yet, polygon of >= 3 vertices, point inside the
//      polygon's bounds): a chunk nobody needs is neither staged nor walked;
//   2. the workgroup stages the chunk's vertices, and the one before them, in LDS;
//   3. every wave walks the chunk's polygons; a polygon none of the wave's lanes needs is skipped (a ballot).  All lanes read the same
//      LDS address per edge (a broadcast, 16 bytes), and the edge's start is the previous edge's end, kept in registers.  The start of
//      a polygon's FIRST edge is its last vertex, which a uniform global load fetches once per polygon and wave.
// A lane's parity bit lives across chunks; it is committed where the polygon ends.  A lane is decided at the first polygon that
// contains it -- the polygon at which the reference's loop returns -- and needs nothing after it.
//
// EXACT: on integer coordinates of magnitude <= 2^24 (the host checks) x < (xj - xi) (y - yi) / (yj - yi) + xi is decided by
// (x - xi) d < (xj - xi) (y - yi) for d = yj - yi > 0, reversed for d < 0.  The differences are integers below 2^25 and the products
// integers below 2^50: float64 holds every one of them exactly, so the integer form is evaluated in float64, on the vertices as
// they are stored, without a division.
constexpr int PIP_TILE = 16;

// the comparison behind the y-test, reached only where that test holds
template <bool EXACT>
__device__ __forceinline__ bool pip_left_of(double x, double y, double xi, double yi, double xj, double yj) {
  if constexpr (EXACT) {
    const double d = yj - yi;
    const double lhs = (x - xi) * d, rhs = (xj - xi) * (y - yi);
    return d > 0.0 ? lhs < rhs : lhs > rhs;
  } else {
    return x < (xj - xi) * (y - yi) / (yj - yi) + xi;
  }
}
// One edge of the walk.  The y-test (yi <= y and y < yj) or (yj <= y and y < yi) costs two comparisons per edge: the two that involve
// yj are the previous edge's (its end is this edge's start), carried in le_j / gt_j.  Most edges fail the test for every lane of the
// wave, and the branch skips the arithmetic.
struct PipEdge {
  double2 vj;
  bool le_j, gt_j;                                                         // yj <= y, y < yj
};
template <bool EXACT>
__device__ __forceinline__ void pip_step(PipEdge& e, const double2 vi, double x, double y, unsigned& c) {
  const bool le_i = vi.y <= y, gt_i = y < vi.y;
  if ((le_i && e.gt_j) || (e.le_j && gt_i)) c ^= (unsigned)pip_left_of<EXACT>(x, y, vi.x, vi.y, e.vj.x, e.vj.y);
  e.vj = vi;
  e.le_j = le_i;
  e.gt_j = gt_i;
}

__device__ __forceinline__ bool pip_in_bounds(const double* __restrict__ bounds, int q, double x, double y) {
  if (!bounds) return true;
  const double* b = bounds + 4 * (size_t)q;
  return x >= b[0] && y >= b[1] && x <= b[2] && y <= b[3];
}
// offsets live in device memory, where the host cannot check them: clamped into the vertex list, so that no entry makes a load leave it
__device__ __forceinline__ int pip_off(const int32_t* __restrict__ off, int q, int V) { return min(max(off[q], 0), V); }

template <bool EXACT>
__global__ __launch_bounds__(256) void points_in_polygons_kernel(const sslcr_pip_desc a, const int tiles_j) {
  __shared__ double2 sv[SSLCR_PIP_CHUNK + 1];                              // sv[k] = vertex base - 1 + k
  const int t = threadIdx.x;
  const double2* __restrict__ verts = reinterpret_cast<const double2*>(a.vertices);
  const int32_t* __restrict__ off = a.offsets;
  const double* __restrict__ bounds = a.bounds;

  // the lane's point
  bool valid;
  int64_t n;
  double x = 0.0, y = 0.0;
  if (a.points) {
    n = (int64_t)blockIdx.x * 256 + t;
    valid = n < a.N;
    if (valid) {
      const double2 p = reinterpret_cast<const double2*>(a.points)[n];
      x = p.x;
      y = p.y;
    }
  } else {
    const int w = t >> 6, l = t & 63;
    const int64_t i = (int64_t)(blockIdx.x / tiles_j) * PIP_TILE + (w >> 1) * 8 + (l >> 3);
    const int64_t j = (int64_t)(blockIdx.x % tiles_j) * PIP_TILE + (w & 1) * 8 + (l & 7);
    valid = i < a.nx && j < a.ny;
    n = i * a.ny + j;
    x = (double)(a.x0 + i * a.step);
    y = (double)(a.y0 + j * a.step);
  }

  bool found = false;
  unsigned c = 0u;                                                         // the parity of the polygon being walked
  int first = -1;
  int p = 0;                                                               // the first polygon that ends after `base`
  for (int base = 0; base < a.V; base += SSLCR_PIP_CHUNK) {
    const int end = min(base + SSLCR_PIP_CHUNK, a.V);
    while (p < a.P && pip_off(off, p + 1, a.V) <= base) ++p;
    // 1. the vote
    bool want = false;
    if (valid && !found) {
      for (int q = p; q < a.P && pip_off(off, q, a.V) < end; ++q)
        if (pip_off(off, q + 1, a.V) - pip_off(off, q, a.V) >= 3 && pip_in_bounds(bounds, q, x, y)) want = true;
    }
    if (!__syncthreads_or(want)) continue;                                 // (the barrier that ends the previous chunk's reads, too)
    // 2. staging
    for (int k = t; k <= SSLCR_PIP_CHUNK; k += 256) {
      const int v = base - 1 + k;
      if (v >= 0 && v < a.V) sv[k] = verts[v];
    }
    __syncthreads();
    // 3. the walk
    for (int q = p; q < a.P && pip_off(off, q, a.V) < end; ++q) {
      const int s = pip_off(off, q, a.V), e = pip_off(off, q + 1, a.V);
      const int v0 = max(s, base), v1 = min(e, end);
      if (v0 >= v1) continue;                                              // an empty polygon
      const bool act = valid && !found && e - s >= 3 && pip_in_bounds(bounds, q, x, y);
      if (v0 == s) c = 0u;
      if (__ballot(act)) {                                                 // wave-uniform
        PipEdge edge;
        edge.vj = v0 == s ? verts[e - 1] : sv[v0 - base];                  // (v0 - 1) - (base - 1)
        edge.le_j = edge.vj.y <= y;
        edge.gt_j = y < edge.vj.y;
        int k = v0 - base + 1;                                             // sv[k] = vertex v0
        const int k1 = v1 - base + 1;
        for (; k + 4 <= k1; k += 4) {                                      // four broadcasts in flight before the first is used
          const double2 a0 = sv[k], a1 = sv[k + 1], a2 = sv[k + 2], a3 = sv[k + 3];
          pip_step<EXACT>(edge, a0, x, y, c);
          pip_step<EXACT>(edge, a1, x, y, c);
          pip_step<EXACT>(edge, a2, x, y, c);
          pip_step<EXACT>(edge, a3, x, y, c);
        }
        for (; k < k1; ++k) pip_step<EXACT>(edge, sv[k], x, y, c);
      }
      if (v1 == e && act && c) {
        found = true;
        first = q;
      }
    }
  }
  if (valid) {
    a.inside[n] = (uint8_t)found;
    if (a.first) a.first[n] = first;
  }
}

hipError_t launch_points_in_polygons(const sslcr_pip_desc& a, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  int64_t blocks;
  int tiles_j = 1;
  if (a.points) {
    blocks = (a.N + 255) / 256;
  } else {
    tiles_j = (a.ny + PIP_TILE - 1) / PIP_TILE;
    blocks = (int64_t)((a.nx + PIP_TILE - 1) / PIP_TILE) * tiles_j;
  }
  if (a.exact) hipLaunchKernelGGL(points_in_polygons_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a, tiles_j);
  else hipLaunchKernelGGL(points_in_polygons_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a, tiles_j);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. thresholded confusion counts
// A wave takes 64 cells at a time; for threshold t (a wave-uniform loop) two ballots count the tissue cells at or above the threshold
// among the tumour and among the normal cells, and LANE t adds the two popcounts to its own registers: nothing is shared while the map
// is read.  At the end the lanes add their counts to the workgroup's LDS counters (32-bit integer atomics; a workgroup sees fewer than
// 2^31 cells), and one thread per counter adds it to the caller's int64 matrix (confusion_flush_cell, as sslcr_predict does).
// Integer sums: any order gives the same counts.
__global__ __launch_bounds__(256) void map_confusion_kernel(const sslcr_map_confusion_desc a) {
  __shared__ unsigned cells[64 * 4];
  const int t = threadIdx.x, lane = t & 63;
  cells[t] = 0u;
  __syncthreads();
  const int64_t n = (int64_t)a.X * a.Y;
  const float* __restrict__ thr = a.thresholds;
  unsigned ge1 = 0u, ge0 = 0u, n1 = 0u, n0 = 0u;                            // lane t: cells >= thr[t] with truth 1 / 0; every lane: the totals
  for (int64_t base = ((int64_t)blockIdx.x * 4 + (t >> 6)) * 64; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t k = base + lane;
    const bool in = k < n && a.tissue[k] != 0;
    const bool tr = in && a.truth[k] != 0;
    const float p = k < n ? a.map[k] : 0.f;
    n1 += (unsigned)__popcll(__ballot(tr));
    n0 += (unsigned)__popcll(__ballot(in && !tr));
    for (int q = 0; q < a.T; ++q) {
      const bool ge = p >= thr[q];
      const unsigned c1 = (unsigned)__popcll(__ballot(tr && ge)), c0 = (unsigned)__popcll(__ballot(in && !tr && ge));
      if (lane == q) {
        ge1 += c1;
        ge0 += c0;
      }
    }
  }
  if (lane < a.T) {                                                        // [t][truth][predicted]
    atomicAdd(&cells[4 * lane + 0], n0 - ge0);
    atomicAdd(&cells[4 * lane + 1], ge0);
    atomicAdd(&cells[4 * lane + 2], n1 - ge1);
    atomicAdd(&cells[4 * lane + 3], ge1);
  }
  __syncthreads();
  if (t < 4 * a.T) confusion_flush_cell(cells, t, a.confusion);
}

hipError_t launch_map_confusion(const sslcr_map_confusion_desc& a, hipStream_t st) {
  const int64_t n = (int64_t)a.X * a.Y;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(map_confusion_kernel, dim3((int)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sslcr
