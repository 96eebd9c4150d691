// fe.hip -- the kernels of the one-way fixed-effects (within) IRLS over the cluster factor (gfx950;
// fe.cpp).  The design is read only by the pass and by cluster.hip's segment sums; the
// kernels here stream the row vectors or the G group rows.
//
// fe_weights_kernel   one workgroup of CLUSTER_TILE_ROWS threads per row tile, thread r = row r of the tile:
//   the row's value (FeKind: working weight, signed score) from rowmath.hpp's reference-order functions --
//   the arithmetic of the pass's own reference rows, at the eta the pass stored and the effective offset
//   o* -- stored to w (zeros on the padding rows and on rows of prior weight 0) and, with its companion
//   (w z), left in LDS; a caller that sums the two values over other row sets (fe2.cpp, over factor 2's
//   lists) has them stored per row as well (FeArgs::va, vb), so no second pass recomputes them.  No
//   segment crosses a tile (cluster_segments), so the tile then sums its own segments, in two fixed steps: pieces (runs of rows within one segment and one block of 8 rows) by the
//   thread of their first row, then each segment's pieces by one thread, both in ascending row order, and
//   the two sums go to Q.  No atomics; the order is a function of (ids, n) alone.  (A serial sum per
//   segment measured 3.8 ms at 10^8 rows in full-tile segments against 2.5 ms in segments of 50: one
//   thread's chain of 128 additions per tile; the two steps bound the chain by 24.)
// fe_offset_kernel    the same tiling: thread j spreads alpha[cluster of segment j] over the segment's rows
//   in LDS, thread r then stores off_r + alpha -- the cluster of a segment is known on the host, so the
//   device holds no per-row id.
// fe_alpha_kernel, fe_scale_kernel   one thread per group (and column): coalesced over the groups.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rowmath.hpp"

namespace sglm {

namespace {

constexpr int FE_NT = CLUSTER_TILE_ROWS;
constexpr int FE_WG_PER_CU = 16;
constexpr int FE_SUB = 8;  // rows per piece of the tile's segment sums
static_assert(FE_NT % 64 == 0 && FE_NT % FE_SUB == 0, "whole waves, whole pieces");
static_assert(FE_NT % RB == 0, "the tiles of n rows cover the ld = n rounded up to RB rows of the per-row outputs");

// w and w z of one row in the reference operation order: the pass's reference rows (rowmath.hpp row_core, the
// links and the variance selected at run time) without their unit deviance, which the pass itself sums.
struct FeWZ {
  double w, wz;
};
__device__ __noinline__ FeWZ fe_row(int fam, int lnk, int mode, double eta, double y, double m, double off, double pw,
                                    double mu0, double theta) {
  const RowCore c = row_core(noncanonical_pair(fam, lnk), fam == FAM_NEGBIN, fam, lnk, mode, eta, m, pw, mu0, theta);
  return FeWZ{c.w, working_wz(c.w, c.eta, y, c.mu, c.g, off)};
}

__global__ void __launch_bounds__(FE_NT) fe_weights_kernel(FeArgs a) {
  __shared__ double sa[FE_NT], sb[FE_NT];
  __shared__ int head[FE_NT];  // 1: the row starts a segment
  const int r = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * FE_NT, row = row0 + r;
    double out = 0.0, va = 0.0, vb = 0.0;
    if (row < a.n) {
      const double pw = a.prior ? a.prior[row] : 1.0;
      if (pw != 0.0) {  // a row of prior weight 0 contributes exact zeros whatever its y and eta
        const double y = a.y[row], m = a.m ? a.m[row] : 1.0;
        if (a.kind == FE_CHECK) {
          if (pw > 0.0) {
            va = y;
            vb = a.family == FAM_BINOMIAL ? m - y : 1.0;
          }
        } else {
          const double eta = a.mode == MODE_IRLS ? a.eta[row] : 0.0;
          if (a.kind == FE_SCORE) {
            const InflRow w = influence_row(a.family, a.link, RESID_WORKING, eta, y, m, pw, a.theta);
            out = va = w.w * w.resid;
          } else {
            const FeWZ w = fe_row(a.family, a.link, a.mode, eta, y, m, a.off ? a.off[row] : 0.0, pw, a.mu0, a.theta);
            out = vb = w.w;
            va = w.wz;
          }
        }
      }
    }
    if (row < a.ld) {  // (the tiles cover every row below ld: ld is n rounded up to RB rows)
      if (a.w) a.w[row] = out;
      if (a.va) a.va[row] = va;
      if (a.vb) a.vb[row] = vb;
    }
    sa[r] = va;
    sb[r] = vb;
    head[r] = 0;
    __syncthreads();
    // The tile's segments are summed in two fixed steps.  A piece is a maximal run of rows inside one
    // segment and one block of FE_SUB rows; the thread of a piece's first row adds the piece in ascending
    // order (at most FE_SUB values), then the thread of a segment adds its pieces in ascending order (at
    // most FE_NT / FE_SUB + 1): a chain of 24 additions where a serial sum of a full-tile segment has 128.
    const int64_t k = a.tile_seg[tile] + r;
    const bool owns = k < a.tile_seg[tile + 1];  // at most FE_NT segments in a tile
    int lo = 0, hi = 0;
    if (owns) {
      lo = (int)(a.seg_start[k] - row0);
      hi = (int)(min(a.seg_start[k + 1], a.n) - row0);
      head[lo] = 1;
    }
    __syncthreads();
    const int nrow = (int)min((int64_t)FE_NT, a.n - row0);
    double p0 = 0.0, p1 = 0.0;
    const bool first = r < nrow && (r % FE_SUB == 0 || head[r]);
    if (first) {
      int i = r;
      do {
        p0 += sa[i];
        p1 += sb[i];
        ++i;
      } while (i < nrow && i % FE_SUB != 0 && !head[i]);
    }
    __syncthreads();  // every piece has read sa / sb
    if (first) {
      sa[r] = p0;
      sb[r] = p1;
    }
    __syncthreads();
    if (owns) {
      double s0 = sa[lo], s1 = sb[lo];
      for (int i = (lo / FE_SUB + 1) * FE_SUB; i < hi; i += FE_SUB) {
        s0 += sa[i];
        s1 += sb[i];
      }
      a.Q[2 * k] = s0;
      a.Q[2 * k + 1] = s1;
    }
    __syncthreads();  // the sums have read sa / sb
  }
}

__global__ void __launch_bounds__(FE_NT) fe_offset_kernel(FeOffsetArgs a) {
  __shared__ double sa[FE_NT];
  const int r = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * FE_NT, row = row0 + r;
    const int64_t k = a.tile_seg[tile] + r;
    if (k < a.tile_seg[tile + 1]) {
      const int lo = (int)(a.seg_start[k] - row0);
      const int hi = (int)(min(a.seg_start[k + 1], a.n) - row0);
      const double v = a.alpha[a.seg_cluster[k]];
      for (int i = lo; i < hi; ++i) sa[i] = v;
    }
    __syncthreads();
    if (row < a.n) a.out[row] = (a.off ? a.off[row] : 0.0) + sa[r];
    else if (row < a.ld) a.out[row] = 0.0;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) fe_alpha_kernel(FeGroupArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.G) return;
  const double W = a.grp[(int64_t)(a.p + 1) * a.ld + g];
  if (!(W > 0.0)) return;  // no row of positive weight: alpha_g is not identified and stays what it was
  double dot = 0.0;
  for (int j = 0; j < a.p; ++j) dot = fma(a.grp[(int64_t)j * a.ld + g], a.beta[j], dot);
  a.alpha[g] += (a.grp[(int64_t)a.p * a.ld + g] - dot) / W;
}

__global__ void __launch_bounds__(256) fe_scale_kernel(FeGroupArgs a) {
  const int64_t total = a.ld * (a.p + 1);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t g = t % a.ld;
    const int j = (int)(t / a.ld);  // j = p: the response
    const double W = (a.meat ? a.grp_w : a.grp)[(int64_t)(a.p + 1) * a.ld + g];
    double v = 0.0;
    if (a.meat) {
      if (j < a.p) {
        v = a.grp[t];
        if (W > 0.0) v -= a.grp[(int64_t)a.p * a.ld + g] * (a.grp_w[t] / W);
      }
    } else if (W > 0.0) {
      v = a.grp[t] * (1.0 / sqrt(W));
    }
    if (j < a.p) a.X[t] = v;
    else a.y[g] = v;
  }
}

}  // namespace

// one workgroup per tile until the device is full: nothing depends on the grid
int fe_grid(int ncu, int64_t ntiles) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)ncu * FE_WG_PER_CU));
}

hipError_t launch_fe_weights(const FeArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if (grid < 1 || !a.y || !a.Q || !a.seg_start || !a.tile_seg || (a.kind != FE_CHECK && !a.w) ||
      (a.kind != FE_CHECK && a.mode == MODE_IRLS && !a.eta))
    return hipErrorInvalidValue;
  hipExtLaunchKernelGGL(fe_weights_kernel, dim3(grid), dim3(FE_NT), 0, st, e0, e1, 0, a);
  return hipGetLastError();
}

hipError_t launch_fe_offset(const FeOffsetArgs& a, int grid, hipStream_t st) {
  if (grid < 1 || !a.alpha || !a.out || !a.seg_cluster) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe_offset_kernel, dim3(grid), dim3(FE_NT), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe_alpha(const FeGroupArgs& a, hipStream_t st) {
  if (a.G < 1 || !a.grp || !a.beta || !a.alpha) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe_alpha_kernel, dim3((unsigned)((a.G + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe_scale(const FeGroupArgs& a, hipStream_t st) {
  if (a.ld < 1 || !a.grp || !a.X || !a.y || (a.meat && !a.grp_w)) return hipErrorInvalidValue;
  const int64_t blocks = (a.ld * (a.p + 1) + 255) / 256;
  hipLaunchKernelGGL(fe_scale_kernel, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sglm
