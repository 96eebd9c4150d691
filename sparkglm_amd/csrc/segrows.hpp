// segrows.hpp -- the row kernel of the steps over the cluster factor (device only; fe.hip, gee.hip; DESIGN.md 4,
// K11): one tiling, one summation order, the row's values from a policy.
//
// One workgroup of CLUSTER_TILE_ROWS threads per row tile, thread r = row r of the tile.  The policy `Row` gives
// the row's NQ values (exact zeros on the padding rows and on rows of prior weight 0) and the one stored to
// SegRowArgs::w.  No segment crosses a tile (cluster_segments), so the tile then sums its own segments from LDS
// in two fixed steps: pieces -- maximal runs of rows inside one segment and one block of SEG_SUB rows -- by the
// thread of their first row, then each segment's pieces by one thread, both in ascending row order, and the NQ
// sums go to Q [nseg][NQ].  No atomics; the order is a function of (ids, n) alone, and it is the bitwise
// definition of every fixed-effects, two-way and GEE result, so it is written here once.  (A serial sum per
// segment measured 3.8 ms at 10^8 rows in full-tile segments against 2.5 ms in segments of 50: one thread's
// chain of 128 additions per tile; the two steps bound the chain by 8 + 16.)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.hpp"

namespace sglm {

constexpr int SEG_NT = CLUSTER_TILE_ROWS;
constexpr int SEG_SUB = 8;  // rows per piece of the tile's segment sums
static_assert(SEG_NT % 64 == 0 && SEG_NT % SEG_SUB == 0, "whole waves, whole pieces");
static_assert(SEG_NT % RB == 0, "the tiles of n rows cover the ld = n rounded up to RB rows of the per-row outputs");

// f(q) for the columns q = 0 .. NQ - 1, q a compile-time constant.  Only the pieces' loop below needs it: an
// unrolled `for q` inside that do-while costs fe_weights_kernel 4 VGPRs and 14 SGPR spills (60 / 30 against the
// 56 / 16 of two named sums), and everywhere else the plain loops give gee_rows_kernel 2 SGPR spills fewer.
template <int NQ, int Q = 0, class F>
__device__ __forceinline__ void each_column(F&& f) {
  if constexpr (Q < NQ) {
    f(std::integral_constant<int, Q>{});
    each_column<NQ, Q + 1>(f);
  }
}

// The segment sums of one tile whose row values thread r holds in v: sv [NQ][SEG_NT] and head [SEG_NT] are the
// workgroup's LDS, free again when it returns.
template <int NQ>
__device__ __forceinline__ void tile_segment_sums(const SegRowArgs& a, int64_t tile, const double (&v)[NQ],
                                                  double (*sv)[SEG_NT], int* head) {
  const int r = threadIdx.x;
  const int64_t row0 = tile * SEG_NT;
#pragma unroll
  for (int q = 0; q < NQ; ++q) sv[q][r] = v[q];
  head[r] = 0;  // 1: the row starts a segment
  __syncthreads();
  const int64_t k = a.tile_seg[tile] + r;
  const bool owns = k < a.tile_seg[tile + 1];  // at most SEG_NT segments in a tile
  int lo = 0, hi = 0;
  if (owns) {
    lo = (int)(a.seg_start[k] - row0);
    hi = (int)(min(a.seg_start[k + 1], a.n) - row0);
    head[lo] = 1;
  }
  __syncthreads();
  const int nrow = (int)min((int64_t)SEG_NT, a.n - row0);
  double pc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) pc[q] = 0.0;
  const bool first = r < nrow && (r % SEG_SUB == 0 || head[r]);
  if (first) {  // at most SEG_SUB values
    int i = r;
    do {
      each_column<NQ>([&](auto q) { pc[q] += sv[q][i]; });
      ++i;
    } while (i < nrow && i % SEG_SUB != 0 && !head[i]);
  }
  __syncthreads();  // every piece has read sv
  if (first) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) sv[q][r] = pc[q];
  }
  __syncthreads();
  if (owns) {  // at most SEG_NT / SEG_SUB + 1 pieces
    double s[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) s[q] = sv[q][lo];
    for (int i = (lo / SEG_SUB + 1) * SEG_SUB; i < hi; i += SEG_SUB) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) s[q] += sv[q][i];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) a.Q[NQ * k + q] = s[q];
  }
  __syncthreads();  // the sums have read sv
}

// The kernel's body.  Row::NQ; Row::values(a, row, pw, v) fills the NQ values of a row of prior weight pw != 0
// and returns the one stored to a.w; Row::store(a, row, v) stores what else the policy keeps per row.
template <class Row>
__device__ __forceinline__ void segment_rows(const SegRowArgs& a) {
  constexpr int NQ = Row::NQ;
  __shared__ double sv[NQ][SEG_NT];
  __shared__ int head[SEG_NT];
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row = tile * SEG_NT + threadIdx.x;
    double out = 0.0, v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = 0.0;
    if (row < a.n) {
      const double pw = a.prior ? a.prior[row] : 1.0;
      if (pw != 0.0) out = Row::values(a, row, pw, v);  // a row of prior weight 0: exact zeros whatever its y and eta
    }
    if (row < a.ld) {  // (the tiles cover every row below ld: ld is n rounded up to RB rows)
      if (a.w) a.w[row] = out;
      Row::store(a, row, v);
    }
    tile_segment_sums<NQ>(a, tile, v, sv, head);
  }
}

}  // namespace sglm
