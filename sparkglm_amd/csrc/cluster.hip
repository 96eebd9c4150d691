// cluster.hip -- sums of score rows over clusters of rows (gfx950): the one primitive the
// cluster-robust covariance (sglm_vcov_cluster; sandwich::vcovCL) adds to the engine.
//
//   S[g, :] = sum_{i: id_i = g} u_i x_i       u: the signed scores (influence.hip, uscore_kernel)
//
// No floating-point atomics: the sums are stored per SEGMENT and then summed per destination, so a
// result depends on (ids, n, p) only -- never on the grid or on timing.
//
// A segment is a maximal run of consecutive rows with one id, cut at every multiple of
// CLUSTER_TILE_ROWS (cluster_segments, the host's rule), so no segment crosses a row tile.
//
// segment_sum_kernel   R[k, j] = sum_{i in segment k} u_i X[i, j], rows in ascending order.
//   The work unit is four consecutive row tiles x a 64-column slab, not a segment: the load is
//   balanced whether a cluster holds one row or ten million.  One wave owns a unit.  It reads the slab 32 rows at a
//   time straight from the column-major design -- lane l loads row l % 32 of column 2 q + l / 32, 256
//   contiguous bytes per half wave and column, every element of X exactly once -- and stores it
//   transposed into LDS, rows padded to 65 doubles: a 16-lane group of the ds_write_b64 then covers
//   the 32 banks once, and the walk's reads (lane = column, one row per step) are consecutive.  The
//   next 32 rows are loaded into registers before the walk of the current ones.  In the walk a lane
//   owns one column and adds u_i x_ij row by row; at the last row of a segment -- the boundaries
//   are per row, uniform across the lanes, so nothing diverges -- it stores its sum to R and
//   starts over.  p < 64: the lanes past the last column idle.
//
// combine_kernel       S[g, j] = the sum of R over cluster g's segments.  The segments, stably ordered
//   by cluster (a CSR the host builds), are cut into chunks of at most CLUSTER_CHUNK = 64 within a
//   cluster; one thread per (chunk, j) adds its chunk's rows in order.  A cluster of one chunk is
//   stored to S at once; the chunks of a larger one go to a scratch whose rows the next level -- the
//   same kernel, the same rule -- adds in turn, until every cluster is one chunk (one level per
//   factor of 64 in the largest cluster's segment count).  A fixed tree, then, in place of a serial
//   sum, which would leave ten clusters of ten million rows to ten times p threads.  S is
//   laid out as a design (column-major, leading dimension ldS, zero padding) for the Gram pass that
//   forms the meat S'S.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace sglm {

namespace {

constexpr int CL_SUB = 32;   // rows staged per step
constexpr int CL_LDW = 65;   // LDS row stride in doubles (64 columns + 1: conflict-free transposing writes)
constexpr int CL_WG_PER_CU = 8;
// row tiles per work unit: the tiles only cut segments, so a unit may walk several in a row and
// restart its load pipeline that much less often
constexpr int CL_UNIT_TILES = 4;
constexpr int CL_UNIT_ROWS = CL_UNIT_TILES * CLUSTER_TILE_ROWS;
static_assert(CLUSTER_TILE_ROWS % CL_SUB == 0 && CL_SUB == RB, "tiles are whole staged steps of one 32-row block");

__global__ void __launch_bounds__(64) segment_sum_kernel(ClusterArgs a) {
  __shared__ double xs[CL_SUB * CL_LDW];
  __shared__ double us[CL_SUB];
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int nslab = (a.p + 63) / 64;
  const int64_t units = (a.ntiles + CL_UNIT_TILES - 1) / CL_UNIT_TILES * nslab;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t tile = unit / nslab * CL_UNIT_TILES;  // the unit's first row tile
    const int c0 = (int)(unit % nslab) * 64;
    const int nc = min(64, a.p - c0);
    const int64_t row0 = tile * CLUSTER_TILE_ROWS;
    const int64_t row1 = min(row0 + (int64_t)CL_UNIT_ROWS, a.n);
    int64_t k = a.tile_seg[tile];
    int64_t end = a.seg_start[k + 1];
    double acc = 0.0;
    // rows [s0, s0 + 32): s0 is a multiple of 32 below n, so every row read lies below ld (the
    // design's and u's zero padding); a column past nc is not read
    double v[32], un;
    const double* xp = a.X + (int64_t)(c0 + h) * a.ld + r;
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = 2 * q + h < nc ? xp[row0 + (int64_t)(2 * q) * a.ld] : 0.0;
    un = a.u[row0 + r];
    for (int64_t s0 = row0; s0 < row1; s0 += CL_SUB) {
      __syncthreads();  // the previous step's walk has read xs / us
#pragma unroll
      for (int q = 0; q < 32; ++q) xs[r * CL_LDW + 2 * q + h] = v[q];
      if (h == 0) us[r] = un;
      __syncthreads();
      const int64_t nxt = s0 + CL_SUB;
      if (nxt < row1) {
#pragma unroll
        for (int q = 0; q < 32; ++q) v[q] = 2 * q + h < nc ? xp[nxt + (int64_t)(2 * q) * a.ld] : 0.0;
        un = a.u[nxt + r];
      }
      const int nr = (int)min((int64_t)CL_SUB, row1 - s0);
      for (int i = 0; i < nr; ++i) {
        acc = fma(us[i], xs[i * CL_LDW + lane], acc);
        if (s0 + i + 1 == end) {  // uniform: the last row of segment k
          if (lane < nc) a.R[k * a.p + c0 + lane] = acc;
          acc = 0.0;
          ++k;
          end = a.seg_start[k + 1];  // (k = nseg reads the sentinel)
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) combine_kernel(CombineArgs a) {
  const int64_t total = a.nchunk * a.p;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t k = t / a.p;
    const int j = (int)(t % a.p);
    const int64_t q1 = a.chunk_start[k + 1];
    double s = 0.0;
    if (a.idx) {
      for (int64_t q = a.chunk_start[k]; q < q1; ++q) s += a.in[a.idx[q] * a.p + j];
    } else {
      for (int64_t q = a.chunk_start[k]; q < q1; ++q) s += a.in[q * a.p + j];
    }
    const int64_t dst = a.chunk_dst[k];
    if (dst >= 0) a.S[dst + (int64_t)j * a.ldS] = s;
    else a.out[(-dst - 1) * a.p + j] = s;
  }
}

}  // namespace

int64_t cluster_segments(const int32_t* ids, int64_t n, int32_t G, int64_t* seg_start, int32_t* seg_cluster) {
  int64_t nseg = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= G) return -1;
    if (i == 0 || ids[i] != ids[i - 1] || i % CLUSTER_TILE_ROWS == 0) {
      if (seg_start) seg_start[nseg] = i;
      if (seg_cluster) seg_cluster[nseg] = ids[i];
      ++nseg;
    }
  }
  if (seg_start) seg_start[nseg] = n;
  return nseg;
}

// one wave per work unit until the device is full: the sums do not depend on the grid
int cluster_sum_grid(int ncu, int64_t n, int p) {
  const int64_t units = (n + CL_UNIT_ROWS - 1) / CL_UNIT_ROWS * ((p + 63) / 64);
  return (int)std::max<int64_t>(1, std::min<int64_t>(units, (int64_t)ncu * CL_WG_PER_CU));
}

hipError_t launch_cluster_sum(const ClusterArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  hipExtLaunchKernelGGL(segment_sum_kernel, dim3(grid), dim3(64), 0, st, e0, e1, 0, a);
  return hipGetLastError();
}

hipError_t launch_cluster_combine(const CombineArgs& a, int ncu, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const int64_t blocks = (a.nchunk * a.p + 255) / 256;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)ncu * 16));
  hipExtLaunchKernelGGL(combine_kernel, dim3(grid), dim3(256), 0, st, e0, e1, 0, a);
  return hipGetLastError();
}

}  // namespace sglm
