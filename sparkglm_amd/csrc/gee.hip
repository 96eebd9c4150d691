// gee.hip -- the kernels of the GEE fits with an exchangeable working correlation over the cluster factor
// (gfx950; gee.cpp).  The design is read only by the pass and by cluster.hip's segment
// sums; the kernels here stream the row vectors or the G group rows.
//
// gee_rows_kernel     segrows.hpp's row kernel with the policy GeeRows.  The row's d = sqrt(w), e = d (y - mu)
//   g'(mu) and d z come from rowmath.hpp's reference-order row_core at the eta the pass stored; d (GEE_SCORE: d e,
//   the signed score) is stored for the segment sums of d x.  d z, 1[pw > 0], e and e^2 are summed per segment
//   into Q [nseg][4] in the tile's two fixed steps.
// gee_moments_kernel  the five moments of the all-reduced group buffer (and the count of groups with rows):
//   thread t of block b adds the groups b 256 + t, + grid 256, ... in that order, the block adds its threads
//   in a fixed tree, and the per-block partials go through reduce_stats_kernel (compensated); n_max, a
//   maximum, is then taken over the same partials by gee_nmax_kernel.  The grid depends on G only.
// gee_scale_kernel    one thread per group and column, coalesced over the groups (as fe_scale_kernel).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rowmath.hpp"
#include "segrows.hpp"

namespace sglm {

namespace {

static_assert(GEE_NM <= NS, "the moments travel in one block of NS scalars");

// d = sqrt(w), d z and e = d (y - mu) g' of one row in the reference operation order (rowmath.hpp row_core)
struct GeeRow {
  double d, dz, e;
};
__device__ __noinline__ GeeRow gee_row(int fam, int lnk, int mode, double eta, double y, double m, double off,
                                       double pw, double mu0, double theta) {
  const RowCore c = row_core(noncanonical_pair(fam, lnk), fam == FAM_NEGBIN, fam, lnk, mode, eta, m, pw, mu0, theta);
  const double d = sqrt(c.w);
  return GeeRow{d, working_wz(d, c.eta, y, c.mu, c.g, off), d * ((y + (-1.0 * c.mu)) * c.g)};
}

// v = d z | 1[pw > 0] | e | e^2 (common.hpp GeeKind)
struct GeeRows {
  static constexpr int NQ = GEE_NQ;
  static __device__ __forceinline__ double values(const SegRowArgs& a, int64_t row, double pw, double (&v)[NQ]) {
    if (pw > 0.0) v[1] = 1.0;
    if (a.kind == GEE_COUNT) return 0.0;
    const double eta = a.mode == MODE_IRLS ? a.eta[row] : 0.0;
    const GeeRow g = gee_row(a.family, a.link, a.mode, eta, a.y[row], a.m ? a.m[row] : 1.0,
                             a.off ? a.off[row] : 0.0, pw, a.mu0, a.theta);
    v[0] = g.dz;
    v[2] = g.e;
    v[3] = g.e * g.e;
    return a.kind == GEE_SCORE ? g.d * g.e : g.d;
  }
  static __device__ __forceinline__ void store(const SegRowArgs&, int64_t, const double (&)[NQ]) {}
};

__global__ void __launch_bounds__(SEG_NT) gee_rows_kernel(SegRowArgs a) { segment_rows<GeeRows>(a); }

__global__ void __launch_bounds__(256) gee_moments_kernel(GroupArgs a) {
  __shared__ double sm[GEE_NM][256];
  const int t = threadIdx.x;
  double v[GEE_NM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double* cn = a.grp + (int64_t)(a.p + 1) * a.ld;
  const double* cE = a.grp + (int64_t)(a.p + 2) * a.ld;
  const double* cQ = a.grp + (int64_t)(a.p + 3) * a.ld;
  for (int64_t g = (int64_t)blockIdx.x * 256 + t; g < a.G; g += (int64_t)gridDim.x * 256) {
    const double n = cn[g], E = cE[g];
    v[M_E2] += E * E;
    v[M_Q] += cQ[g];
    v[M_PAIRS] += 0.5 * (n * (n - 1.0));
    v[M_N] += n;
    v[M_NMAX] = fmax(v[M_NMAX], n);
    v[M_GEFF] += n > 0.0 ? 1.0 : 0.0;
  }
#pragma unroll
  for (int q = 0; q < GEE_NM; ++q) sm[q][t] = v[q];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int q = 0; q < GEE_NM; ++q)
        sm[q][t] = q == M_NMAX ? fmax(sm[q][t], sm[q][t + s]) : sm[q][t] + sm[q][t + s];
    }
    __syncthreads();
  }
  if (t < NS) a.partials[(int64_t)blockIdx.x * NS + t] = t < GEE_NM ? sm[t][0] : 0.0;
}

// out[M_NMAX] = the maximum of the blocks' maxima (reduce_stats_kernel left their sum there)
__global__ void __launch_bounds__(256) gee_nmax_kernel(const double* part, int nparts, double* out) {
  __shared__ double sm[256];
  const int t = threadIdx.x;
  double v = 0.0;
  for (int b = t; b < nparts; b += 256) v = fmax(v, part[(int64_t)b * NS + M_NMAX]);
  sm[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sm[t] = fmax(sm[t], sm[t + s]);
    __syncthreads();
  }
  if (t == 0) out[M_NMAX] = sm[0];
}

__global__ void __launch_bounds__(256) gee_scale_kernel(GroupArgs a) {
  const int64_t total = a.ld * (a.p + 1);
  const double omr = 1.0 - a.rho;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t g = t % a.ld;
    const int j = (int)(t / a.ld);  // j = p: the response
    const double n = a.grp2[(int64_t)(a.p + 1) * a.ld + g];
    double v = 0.0;
    if (n > 0.0) {
      const double c = a.rho / (omr + n * a.rho);
      if (a.meat) {
        if (j < a.p) v = (a.grp[t] - (c * a.grp2[(int64_t)(a.p + 2) * a.ld + g]) * a.grp2[t]) / omr;
      } else {
        v = sqrt(fabs(c)) * a.grp[t];
      }
    }
    if (j < a.p) a.X[t] = v;
    else a.y[g] = v;
  }
}

}  // namespace

int gee_moment_grid(int64_t G) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((G + 255) / 256, GEE_MOMENT_BLOCKS));
}

hipError_t launch_gee_rows(const SegRowArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if (grid < 1 || !a.Q || !a.seg_start || !a.tile_seg || (a.kind != GEE_COUNT && (!a.w || !a.y)) ||
      (a.kind != GEE_COUNT && a.mode == MODE_IRLS && !a.eta))
    return hipErrorInvalidValue;
  hipExtLaunchKernelGGL(gee_rows_kernel, dim3(grid), dim3(SEG_NT), 0, st, e0, e1, 0, a);
  return hipGetLastError();
}

hipError_t launch_gee_moments(const GroupArgs& a, double* out, hipStream_t st) {
  if (a.G < 1 || a.ld < a.G || !a.grp || !a.partials || !out) return hipErrorInvalidValue;
  const int grid = gee_moment_grid(a.G);
  hipLaunchKernelGGL(gee_moments_kernel, dim3(grid), dim3(256), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (hipError_t e = launch_reduce_stats(a.partials, grid, out, st); e != hipSuccess) return e;
  hipLaunchKernelGGL(gee_nmax_kernel, dim3(1), dim3(256), 0, st, a.partials, grid, out);
  return hipGetLastError();
}

hipError_t launch_gee_scale(const GroupArgs& a, hipStream_t st) {
  if (a.ld < 1 || !a.grp || !a.grp2 || !a.X || !a.y) return hipErrorInvalidValue;
  const int64_t blocks = (a.ld * (a.p + 1) + 255) / 256;
  hipLaunchKernelGGL(gee_scale_kernel, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sglm
