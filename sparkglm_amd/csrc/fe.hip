// fe.hip -- the kernels of the one-way fixed-effects (within) IRLS over the cluster factor (gfx950;
// fe.cpp).  The design is read only by the pass and by cluster.hip's segment sums; the
// kernels here stream the row vectors or the G group rows.
//
// fe_weights_kernel   segrows.hpp's row kernel with the policy FeRows: the row's value (FeKind: working weight,
//   signed score) from rowmath.hpp's reference-order functions -- the arithmetic of the pass's own reference
//   rows, at the eta the pass stored and the effective offset o* -- stored to w, and with its companion (w z)
//   summed per segment into Q [nseg][2] in the tile's two fixed steps; a caller that sums the two values over
//   other row sets (fe2.cpp, over factor 2's lists) has them stored per row as well (SegRowArgs::va, vb), so no
//   second pass recomputes them.
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
#include "segrows.hpp"

namespace sglm {

namespace {

constexpr int FE_NT = SEG_NT;
constexpr int FE_WG_PER_CU = 16;

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

// v = {va, vb}: w z | u | y and w | 0 | m - y or 1 (common.hpp FeKind)
struct FeRows {
  static constexpr int NQ = 2;
  static __device__ __forceinline__ double values(const SegRowArgs& a, int64_t row, double pw, double (&v)[NQ]) {
    const double y = a.y[row], m = a.m ? a.m[row] : 1.0;
    double out = 0.0;
    if (a.kind == FE_CHECK) {
      if (pw > 0.0) {
        v[0] = y;
        v[1] = a.family == FAM_BINOMIAL ? m - y : 1.0;
      }
    } else {
      const double eta = a.mode == MODE_IRLS ? a.eta[row] : 0.0;
      if (a.kind == FE_SCORE) {
        const InflRow w = influence_row(a.family, a.link, RESID_WORKING, eta, y, m, pw, a.theta);
        out = v[0] = w.w * w.resid;
      } else {
        const FeWZ w = fe_row(a.family, a.link, a.mode, eta, y, m, a.off ? a.off[row] : 0.0, pw, a.mu0, a.theta);
        out = v[1] = w.w;
        v[0] = w.wz;
      }
    }
    return out;
  }
  static __device__ __forceinline__ void store(const SegRowArgs& a, int64_t row, const double (&v)[NQ]) {
    if (a.va) a.va[row] = v[0];
    if (a.vb) a.vb[row] = v[1];
  }
};

__global__ void __launch_bounds__(FE_NT) fe_weights_kernel(SegRowArgs a) { segment_rows<FeRows>(a); }

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

__global__ void __launch_bounds__(256) fe_alpha_kernel(GroupArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.G) return;
  const double W = a.grp[(int64_t)(a.p + 1) * a.ld + g];
  if (!(W > 0.0)) return;  // no row of positive weight: alpha_g is not identified and stays what it was
  double dot = 0.0;
  for (int j = 0; j < a.p; ++j) dot = fma(a.grp[(int64_t)j * a.ld + g], a.beta[j], dot);
  a.alpha[g] += (a.grp[(int64_t)a.p * a.ld + g] - dot) / W;
}

__global__ void __launch_bounds__(256) fe_scale_kernel(GroupArgs a) {
  const int64_t total = a.ld * (a.p + 1);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t g = t % a.ld;
    const int j = (int)(t / a.ld);  // j = p: the response
    const double W = (a.meat ? a.grp2 : a.grp)[(int64_t)(a.p + 1) * a.ld + g];
    double v = 0.0;
    if (a.meat) {
      if (j < a.p) {
        v = a.grp[t];
        if (W > 0.0) v -= a.grp[(int64_t)a.p * a.ld + g] * (a.grp2[t] / W);
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

hipError_t launch_fe_weights(const SegRowArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
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

hipError_t launch_fe_alpha(const GroupArgs& a, hipStream_t st) {
  if (a.G < 1 || !a.grp || !a.beta || !a.alpha) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe_alpha_kernel, dim3((unsigned)((a.G + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe_scale(const GroupArgs& a, hipStream_t st) {
  if (a.ld < 1 || !a.grp || !a.X || !a.y || (a.meat && !a.grp2)) return hipErrorInvalidValue;
  const int64_t blocks = (a.ld * (a.p + 1) + 255) / 256;
  hipLaunchKernelGGL(fe_scale_kernel, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sglm
