// influence.hip -- per-row diagnostics of a resident design with p <= 256 (gfx950).
//
//   q_i = x_i' C x_i,  C = inv(X'WX)      the row quadratic form (leverage h = w q, se.fit = sqrt(phi q))
//
// The Gram kernels' MFMA with the roles transposed: k runs over COLUMNS, one operand is X, the
// other a 16 x 16 block of C.  C is symmetric, so only the block triangle c <= b is multiplied,
// with the off-diagonal blocks doubled on the host (C~, influence_tiles):
//   q_i = sum_b sum_{c <= b} x_ic' C~_cb x_ib
// -- P16 (P16 + 1) / 2 tiles, as many fp64 MFMA flops per row as the Gram pass.
//
// One wave owns 16 rows (RS row blocks of 16 each).  Per column block c and k-step s it holds
//   xv[c][s] = X[row l % 16, column 16 c + 4 s + l / 16]
// which is the B operand of v_mfma_f64_16x16x4_f64 (B[k = l / 16][n = l % 16]) of the transposed
// product T_b' = sum_{c <= b} C~_cb' X_c' (A = C~_cb', 16 x 4 per step: lane l holds
// C~[16 c + 4 s + l / 16][16 b + l % 16]).  Its result D[m][n] = T[row n][column 16 b + m] comes
// out with lane l, register v holding m = l / 16 + 4 v, n = l % 16 -- the column 16 b + 4 v + l / 16
// of row l % 16, exactly the element xv[b][v] the same lane already holds.  So the design is read
// from HBM once, straight into registers (16 lanes x 8 B = 128 B contiguous per column), serves as
// MFMA operand, as the factor of the row reduction rowsum(T_b o X_b) and as the eta = x'beta
// operand, and the reduction needs no data movement beyond one sum over the four lane groups.
//
// C~ reaches the waves through LDS: for block column b the workgroup copies the b + 1 tiles (c, b)
// (contiguous in the host's tile order, <= 32 KB) from global memory -- C~ is <= 272 KB and stays in
// L2 -- prefetched into registers one block column ahead, so the L2 latency hides behind the MFMAs.
// A workgroup step covers 64 * RS rows; C~ is re-read from L2 once per step.
//
// score_kernel is the same body writing one vector, the sandwich covariance's score weights
//   omega_i = u_i^2 / (1 - h_i)^k,  u_i = w_i (y_i - mu_i) g'(mu_i),  h_i = w_i q_i
// (k = 0: no MFMA product), which the engine then feeds to a Gram pass as prior weights.
// uscore_kernel stores u_i itself, the factor of the cluster sums of cluster.hip.
//
// firth_kernel is the body's fifth mode: Firth's adjusted score g* = sum_i v_i x_i, v_i = u_i + h_i r_i / 2, in
// the same read of X.  The lane that holds X[row i][16 c + 4 s + g] in xv[r][c][s] accumulates v_i times it in
// gacc[c][s] -- the column sums need no data movement either -- across the workgroup's steps; at the end the 16
// lanes of a lane group, then the four waves (through LDS), are summed in a fixed order into one partial p-vector
// per workgroup, and infl_sum_kernel adds the workgroups' partials.  Past FIRTH_FUSED_MAX column blocks the
// accumulators do not fit beside the design's registers: there the mode stores v and firth_xtv_kernel streams X
// a second time for X'v, a lane per row, into the same partials.
//
// The host side is written once for every mode (enum InflMode, common.hpp): launch_infl, the grid rule
// infl_grid -- whose rows per step are the body's own infl_step -- and the fixed-order sum launch_infl_sum of
// the workgroups' partials (the leverage sum: one column).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rowmath.hpp"

namespace sglm {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int INFL_NW = 4;            // waves per workgroup
constexpr int INFL_NT = 64 * INFL_NW;
// row blocks of 16 per wave: two while the kernel stays within 256 VGPRs without scratch (P16 <= 7;
// two workgroups per CU, and no AGPRs: the fp64 MFMA's AGPR form runs at 60 %).
// The Firth mode: one at every width (its accumulators take the second block's registers).
constexpr int infl_rs(int mode, int P16) { return mode != INFL_FIRTH && P16 <= 7 ? 2 : 1; }
// rows per workgroup step: the body's and (firth_xtv_kernel: the Firth mode's) the grid rule's
constexpr int infl_step(int mode, int P16) { return 16 * infl_rs(mode, P16) * INFL_NW; }
constexpr int infl_wg_per_cu(int P16) { return P16 <= 4 ? 4 : 2; }

__device__ __forceinline__ double group_sum(double v) {  // over the four lane groups l / 16
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// The Firth mode: fused (g* in the same read of X) up to FIRTH_FUSED_MAX column blocks, v stored for
// firth_xtv_kernel above.
// (VGPRs of the fused form, no scratch: 225 / 243 / 255 at P16 = 8 / 9 / 10; P16 = 11 spills)
constexpr int FIRTH_FUSED_MAX = 10;
constexpr bool firth_fused(int P16) { return P16 <= FIRTH_FUSED_MAX; }

// The accumulators gacc[c][s] (column 16 c + 4 s + g, the rows of lane i) of a workgroup into its partial: the 16
// lanes of each lane group, then the four waves through LDS (red [INFL_NW][16 P16]), each in a fixed order.
// Columns >= p are never stored.
template <int P16>
__device__ __forceinline__ void firth_reduce(double (&gacc)[P16][4], double* red, double* part, int p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  __syncthreads();  // red may be the MFMA operand panel: every wave is done reading it
#pragma unroll
  for (int c = 0; c < P16; ++c)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double t = gacc[c][s];
      t += __shfl_xor(t, 1);
      t += __shfl_xor(t, 2);
      t += __shfl_xor(t, 4);
      t += __shfl_xor(t, 8);
      if (i == 0) red[wave * (16 * P16) + 16 * c + 4 * s + g] = t;
    }
  __syncthreads();
  for (int col = tid; col < p; col += INFL_NT) {
    double t = red[col];
    for (int k = 1; k < INFL_NW; ++k) t += red[k * (16 * P16) + col];
    part[col] = t;
  }
}

template <int P16, int MODE>
__device__ __forceinline__ void influence_body(const InflArgs& a) {
  constexpr bool ROWS = MODE != INFL_QFORM;
  constexpr bool FIRTH = MODE == INFL_FIRTH;
  constexpr bool GACC = FIRTH && firth_fused(P16);  // the adjusted score accumulates in this kernel
  constexpr int RS = infl_rs(MODE, P16);
  constexpr int STEP = infl_step(MODE, P16);                     // rows per workgroup step
  constexpr int PF = (P16 * INFL_TILE + INFL_NT - 1) / INFL_NT;  // prefetch registers per thread
  __shared__ double panel[P16 * INFL_TILE];
  __shared__ double sbeta[16 * P16];
  __shared__ double swave[INFL_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  if (ROWS) {
    for (int c = tid; c < 16 * P16; c += INFL_NT) sbeta[c] = c < a.p ? a.beta[c] : 0.0;
    __syncthreads();
  }
  const bool need_q = a.need_q != 0;
  double pf[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) pf[k] = 0.0;
  if (need_q) pf[0] = a.ct[tid];  // block column 0: one tile
  double hsum = 0.0;
  double gacc[GACC ? P16 : 1][4];
  if constexpr (GACC) {
#pragma unroll
    for (int c = 0; c < P16; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) gacc[c][s] = 0.0;
  }
  const int64_t nsteps = (a.n + STEP - 1) / STEP;
  for (int64_t step = blockIdx.x; step < nsteps; step += gridDim.x) {
    double xv[RS][P16][4];
    int64_t row[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      row[r] = step * STEP + (int64_t)((wave * RS + r) * 16 + i);
      // Unconditional loads from clamped addresses: a row >= n reads row n - 1 (its results are never
      // stored; an MFMA column and a lane's sums belong to one row, so nothing crosses rows), a column
      // >= p reads column p - 1 -- only the last column block can hold one (p > 16 (P16 - 1)) -- and
      // meets the zeros of C~ and beta there.  Masked loads would keep 4 P16 masks live.
      const int64_t rr = row[r] < a.n ? row[r] : a.n - 1;
      // the blocks before the last: one running pointer (column 4 u + g, u = 4 c + s), one 64-bit add per load
      const int64_t ld = a.ld;
      const double* xp = a.X + rr + (int64_t)g * ld;
      const int64_t ld4 = 4 * ld;
#pragma unroll
      for (int c = 0; c < P16 - 1; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          xv[r][c][s] = *xp;
          xp += ld4;
        }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int col = min(16 * (P16 - 1) + 4 * s + g, a.p - 1);
        xv[r][P16 - 1][s] = a.X[rr + (int64_t)col * ld];
      }
    }
    double eta[RS], q[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) eta[r] = q[r] = 0.0;
    if (ROWS) {
      // (the index is made opaque per step: beta is loop-invariant, and hoisted out of the step loop
      // its 4 P16 values per lane would hold 8 P16 VGPRs next to the design's)
      int gb = g;
      asm volatile("" : "+v"(gb));
#pragma unroll
      for (int c = 0; c < P16; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double bv = sbeta[16 * c + 4 * s + gb];
#pragma unroll
          for (int r = 0; r < RS; ++r) eta[r] = fma(xv[r][c][s], bv, eta[r]);
        }
#pragma unroll
      for (int r = 0; r < RS; ++r) eta[r] = group_sum(eta[r]);
    }
    if (need_q) {
#pragma unroll
      for (int b = 0; b < P16; ++b) {
        __syncthreads();  // the previous block column's tiles are consumed
#pragma unroll
        for (int k = 0; k < PF; ++k)
          if (k * INFL_NT < (b + 1) * INFL_TILE) panel[k * INFL_NT + tid] = pf[k];
        __syncthreads();
        {  // the next block column (the first one of the next step after the last)
          const int nb = (b + 1 < P16) ? b + 1 : 0;
          // (the scalar base is made opaque: the tiles' offsets exceed the loads' immediate field, and
          // the compiler otherwise keeps one precomputed 64-bit address per tile live -- T pairs)
          const double* src = a.ct + (int64_t)(nb * (nb + 1) / 2) * INFL_TILE;
          asm volatile("" : "+s"(src));
#pragma unroll
          for (int k = 0; k < PF; ++k)
            if (k * INFL_NT < (nb + 1) * INFL_TILE) pf[k] = src[k * INFL_NT + tid];
        }
        d4 acc[RS][2];
#pragma unroll
        for (int r = 0; r < RS; ++r) acc[r][0] = acc[r][1] = d4{0.0, 0.0, 0.0, 0.0};
        // tile c + 1's operands are read from LDS before tile c's MFMAs issue; the scheduling barrier
        // keeps the compiler from hoisting the whole block column's reads (8 (b + 1) VGPRs) instead
        double av[2][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[0][s] = panel[s * 64 + lane];
#pragma unroll
        for (int c = 0; c <= b; ++c) {
          if (c < b) {
#pragma unroll
            for (int s = 0; s < 4; ++s) av[(c + 1) & 1][s] = panel[(c + 1) * INFL_TILE + s * 64 + lane];
          }
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < RS; ++r)
              acc[r][s & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[c & 1][s], xv[r][c][s], acc[r][s & 1], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < RS; ++r)
#pragma unroll
          for (int v = 0; v < 4; ++v) q[r] = fma(acc[r][0][v] + acc[r][1][v], xv[r][b][v], q[r]);
      }
#pragma unroll
      for (int r = 0; r < RS; ++r) q[r] = group_sum(q[r]);
    }
    if constexpr (FIRTH) {
      // v = u + h r / 2 on lane group 0, exactly 0 for a row >= n (whose registers hold row n - 1) and for a row
      // of prior weight 0; then from lane i of group 0 to the four lanes that hold row i's columns
      double v = 0.0;
      if (g == 0 && row[0] < a.n) {
        const int64_t ri = row[0];
        const double e = eta[0] + (a.off ? a.off[ri] : 0.0);
        const double pw = a.prior ? a.prior[ri] : 1.0;
        const FirthRow w = firth_row(a.family, a.link, e, a.y[ri], a.m ? a.m[ri] : 1.0, pw);
        const double h = w.w * q[0];
        if (a.hat) a.hat[ri] = h;
        hsum += h;
        v = pw == 0.0 ? 0.0 : w.u + (0.5 * h) * w.r;
        if constexpr (!GACC) a.out[ri] = v;
      }
      if constexpr (GACC) {
        v = __shfl(v, i);
#pragma unroll
        for (int c = 0; c < P16; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s) gacc[c][s] = fma(v, xv[0][c][s], gacc[c][s]);
      }
      continue;
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      if (g != 0 || row[r] >= a.n) continue;  // 16 lanes store 16 consecutive rows
      const int64_t ri = row[r];
      if (!ROWS) {
        a.out[ri] = sqrt(fmax(0.0, a.dispersion * q[r]));
        continue;
      }
      const double e = eta[r] + (a.off ? a.off[ri] : 0.0);
      if constexpr (MODE == INFL_SCORE || MODE == INFL_USCORE) {
        // u = w (y - mu) g'(mu): the working weight times the working residual; a row of prior weight
        // 0 contributes exactly 0 whatever its mu
        const double pw = a.prior ? a.prior[ri] : 1.0;
        const InflRow w = influence_row(a.family, a.link, RESID_WORKING, e, a.y[ri], a.m ? a.m[ri] : 1.0, pw,
                                        a.theta);
        const double u = w.w * w.resid;
        if constexpr (MODE == INFL_USCORE) {
          a.out[ri] = pw == 0.0 ? 0.0 : u;
          continue;
        }
        double om = u * u;
        if (a.hc_k > 0) {
          const double d = 1.0 - w.w * q[r];
          om /= a.hc_k > 1 ? d * d : d;
        }
        a.out[ri] = pw == 0.0 ? 0.0 : om;
        continue;
      }
      const InflRow w = influence_row(a.family, a.link, a.resid_type, e, a.y[ri], a.m ? a.m[ri] : 1.0,
                                      a.prior ? a.prior[ri] : 1.0, a.theta);
      const double h = w.w * q[r];
      if (a.resid) a.resid[ri] = w.resid;
      if (a.hat) a.hat[ri] = h;
      if (a.cooks) {
        const double t = w.rp / (1.0 - h);
        a.cooks[ri] = (t * t) * h / (a.dispersion * (double)a.p);
      }
      hsum += h;
    }
  }
  if (FIRTH || (MODE == INFL_ROWS && a.hpart)) {
    // the workgroup's sum of h: lanes, then waves, in a fixed order.  The Firth mode's partial [p + 1]: the
    // adjusted score (fused widths), then the sum of h
    double* part = FIRTH ? a.gpart + (int64_t)blockIdx.x * (a.p + 1) : a.hpart + blockIdx.x;
    hsum += __shfl_xor(hsum, 1);
    hsum += __shfl_xor(hsum, 2);
    hsum += __shfl_xor(hsum, 4);
    hsum += __shfl_xor(hsum, 8);
    if (lane == 0) swave[wave] = hsum;
    if constexpr (GACC) {
      static_assert(INFL_NW * 16 <= INFL_TILE, "the wave partials fit the operand panel");
      firth_reduce<P16>(gacc, panel, part, a.p);
    } else {
      __syncthreads();
    }
    if (tid == 0) {
      double s = swave[0];
      for (int k = 1; k < INFL_NW; ++k) s += swave[k];
      part[FIRTH ? a.p : 0] = s;
    }
  }
}

template <int P16>
__global__ void __launch_bounds__(INFL_NT, 2) influence_kernel(InflArgs a) {
  influence_body<P16, INFL_ROWS>(a);
}
template <int P16>
__global__ void __launch_bounds__(INFL_NT, 2) qform_kernel(InflArgs a) {
  influence_body<P16, INFL_QFORM>(a);
}
template <int P16>
__global__ void __launch_bounds__(INFL_NT, 2) score_kernel(InflArgs a) {
  influence_body<P16, INFL_SCORE>(a);
}
template <int P16>
__global__ void __launch_bounds__(INFL_NT, 2) uscore_kernel(InflArgs a) {
  influence_body<P16, INFL_USCORE>(a);
}

template <int P16>
__global__ void __launch_bounds__(INFL_NT, 2) firth_kernel(InflArgs a) {
  influence_body<P16, INFL_FIRTH>(a);
}

// X'v of the stored v (a.out), the widths past FIRTH_FUSED_MAX: a second stream of X over firth_kernel's steps
// and grid, into the first p entries of the same partials.  No MFMA operand layout binds here, so a lane is a row:
// a step's 64 rows are the 64 lanes of every wave (512 contiguous bytes per column and load), wave w owns the
// 4 P16 columns from 4 P16 w on and carries one accumulator per column across the steps; at the end each column
// is summed over the 64 lanes in a fixed order.
template <int P16>
__global__ void __launch_bounds__(INFL_NT, 2) firth_xtv_kernel(InflArgs a) {
  constexpr int CW = 4 * P16;  // columns per wave
  constexpr int FIRTH_STEP = infl_step(INFL_FIRTH, P16);  // firth_kernel's steps
  static_assert(FIRTH_STEP == 64, "a step is one row per lane");
  const int lane = threadIdx.x & 63;
  const int col0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * CW;
  double gacc[CW];
#pragma unroll
  for (int k = 0; k < CW; ++k) gacc[k] = 0.0;
  const int64_t ld = a.ld;
  const int64_t nsteps = (a.n + FIRTH_STEP - 1) / FIRTH_STEP;
  for (int64_t step = blockIdx.x; step < nsteps; step += gridDim.x) {
    const int64_t row = step * FIRTH_STEP + lane;
    const int64_t rr = row < a.n ? row : a.n - 1;  // clamped as in influence_body: v, not x, is masked
    const double v = row < a.n ? a.out[rr] : 0.0;
    // a column >= p reads column p - 1 (never stored): the pointer stops advancing there
    const double* xp = a.X + rr + (int64_t)min(col0, a.p - 1) * ld;
    // four batches of P16 loads, batch b + 1 issued before batch b's products: up to 2 P16 x 512 bytes per wave
    // in flight (the scheduling barrier keeps the compiler from sinking the loads to their uses)
    double x[2][P16];
#pragma unroll
    for (int b = 0; b <= 4; ++b) {
      if (b < 4) {
#pragma unroll
        for (int j = 0; j < P16; ++j) {
          x[b & 1][j] = *xp;
          xp += (col0 + b * P16 + j + 1 < a.p) ? ld : 0;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (b > 0) {
#pragma unroll
        for (int j = 0; j < P16; ++j)
          gacc[(b - 1) * P16 + j] = fma(v, x[(b - 1) & 1][j], gacc[(b - 1) * P16 + j]);
      }
    }
  }
  double* part = a.gpart + (int64_t)blockIdx.x * (a.p + 1);
#pragma unroll
  for (int k = 0; k < CW; ++k) {
    double t = gacc[k];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    t += __shfl_xor(t, 16);
    t += __shfl_xor(t, 32);
    if (lane == 0 && col0 + k < a.p) part[col0 + k] = t;
  }
}

// out[j] = the sum over the workgroups' partials part[k][j] (stride doubles apart), one workgroup per entry:
// 256 strided sums, then those in order
__global__ void __launch_bounds__(256) infl_sum_kernel(const double* __restrict__ part, int nparts, int stride,
                                                       double* __restrict__ out) {
  __shared__ double ss[256];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < nparts; k += 256) s += part[(int64_t)k * stride + j];
  ss[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = ss[0];
    for (int k = 1; k < 256; ++k) t += ss[k];
    out[j] = t;
  }
}

// The kernels of one width, by mode; xtv: the Firth mode's second kernel, null at the fused widths (where it
// is not built)
typedef void (*InflKernel)(InflArgs);
struct WidthKernels {
  InflKernel mode[5], xtv;
};
template <int N>
WidthKernels width_kernels() {
  static_assert(INFL_ROWS == 0 && INFL_QFORM == 1 && INFL_SCORE == 2 && INFL_USCORE == 3 && INFL_FIRTH == 4);
  WidthKernels k{{influence_kernel<N>, qform_kernel<N>, score_kernel<N>, uscore_kernel<N>, firth_kernel<N>}, nullptr};
  if constexpr (!firth_fused(N)) k.xtv = firth_xtv_kernel<N>;
  return k;
}

// the only list of the widths; null: no such width or mode
const WidthKernels* kernels_of(int mode, int P16) {
#define K(N) width_kernels<N>()
  static const WidthKernels all[MAX_P16] = {K(1), K(2),  K(3),  K(4),  K(5),  K(6),  K(7),  K(8),
                                            K(9), K(10), K(11), K(12), K(13), K(14), K(15), K(16)};
#undef K
  return mode >= INFL_ROWS && mode <= INFL_FIRTH && P16 >= 1 && P16 <= MAX_P16 ? &all[P16 - 1] : nullptr;
}

}  // namespace

// One workgroup per resident slot (capped at infl_wg_per_cu): the grid -- and with it the order of the sum of h
// and of the Firth partials -- depends on the mode, the shape and the device only.  The two Firth kernels share
// it: the second fills the first's partials.
int infl_grid(int mode, int P16, int ncu, int64_t n) {
  // workgroups of the kernel one CU holds (registers and LDS: the runtime's own count): the Firth mode's of
  // firth_kernel, every other mode's of influence_kernel
  const WidthKernels* k = kernels_of(mode, P16);
  int wgs = 1;
  if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, k->mode[mode == INFL_FIRTH ? INFL_FIRTH : INFL_ROWS],
                                                         INFL_NT, 0) != hipSuccess || wgs < 1)
    wgs = 1;
  wgs = std::min(wgs, infl_wg_per_cu(P16));
  const int64_t step = infl_step(mode, P16);
  const int64_t steps = std::min<int64_t>((n + step - 1) / step, (int64_t)1 << 30);
  return std::max(1, (int)std::min<int64_t>(steps, (int64_t)ncu * wgs));
}

bool firth_is_fused(int P16) { return firth_fused(P16); }

void influence_tiles(const double* C, int p, double* out) {
  const int P16 = (p + 15) / 16;
  for (int b = 0; b < P16; ++b)
    for (int c = 0; c <= b; ++c) {
      double* t = out + (int64_t)(b * (b + 1) / 2 + c) * INFL_TILE;
      const double f = c == b ? 1.0 : 2.0;
      for (int s = 0; s < 4; ++s)
        for (int l = 0; l < 64; ++l) {
          const int r = 16 * c + 4 * s + (l >> 4), cc = 16 * b + (l & 15);
          t[s * 64 + l] = (r < p && cc < p) ? f * C[r + (int64_t)cc * p] : 0.0;
        }
    }
}

hipError_t launch_infl(int mode, int P16, const InflArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const WidthKernels* k = kernels_of(mode, P16);
  if (!k) return hipErrorInvalidValue;
  const dim3 g(grid), b(INFL_NT);
  if (mode == INFL_FIRTH && k->xtv) {  // two launches between the events: the rows (v stored), then X'v
    hipExtLaunchKernelGGL(k->mode[mode], g, b, 0, st, e0, nullptr, 0, a);
    hipExtLaunchKernelGGL(k->xtv, g, b, 0, st, nullptr, e1, 0, a);
  } else {
    hipExtLaunchKernelGGL(k->mode[mode], g, b, 0, st, e0, e1, 0, a);
  }
  return hipGetLastError();
}

hipError_t launch_infl_sum(const double* part, int nparts, int ncol, double* out, hipStream_t st) {
  return launch_part_sum(part, nparts, ncol, ncol, out, st);
}

hipError_t launch_part_sum(const double* part, int nparts, int stride, int ncol, double* out, hipStream_t st) {
  hipLaunchKernelGGL(infl_sum_kernel, dim3(ncol), dim3(256), 0, st, part, nparts, stride, out);
  return hipGetLastError();
}

}  // namespace sglm
