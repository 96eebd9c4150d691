// narrow_core.hpp -- what the narrow pass kernels share whatever the storage of X: device code only,
// included by narrow.hip (fp64 X) and narrow_f32.hip (float X) and by nothing else.
//
// Each kernel keeps its geometry, LDS image and bank argument, DMA staging, eta formation, wait
// accounting, block loops and launcher.  Only pieces whose move leaves every kernel's register, scratch
// and LDS figures at what they were are here (profiles/narrow_core_isa.txt).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"
#include "rowmath.hpp"
#include "waitcnt.hpp"

namespace sglm {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

// Issue priority by phase: a wave runs its row stage (eta, the family arithmetic: a dependent fp64
// chain) at high priority and its Grams at low, so the partner wave's MFMA stream fills the row
// stage's latencies instead of delaying its instructions (round 5: p = 32 -2 %, p = 48 -1 %, p = 64
// +-0 against priorities alternating between the two waves every 4 blocks; 12 waves a CU on 8-row
// blocks at p > 32: +18-20 %, DESIGN.md 4 K1').  Measured and not kept: the diagonal tiles on three
// v_mfma_f64_4x4x4f64 (rotated B operands from LDS or by DPP: slower at p = 32 and 64); a
// batched Gram phase (all operands, then all VALU, then all MFMAs per block: p = 64 +25 %).
constexpr int PRIO_ROWS = 2, PRIO_GRAM = 0;

__device__ __forceinline__ double xor16_sum(double v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}
__device__ __forceinline__ double xor32_sum(double v) {
  const auto a = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}

// Lane l of a 16-lane row takes the value of lane l & ~12 (the first 4-lane group's lane of the same
// position): ds_swizzle in bit mode, and_mask 0b10011 on the lane id within 32.
__device__ __forceinline__ double bcast_quad0(double v) {
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x13);
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x13);
  return __hiloint2double(hi, lo);
}

// One k-step (4 rows) of the lower-triangular Gram on v_mfma_f64_16x16x4_f64.
// T4 (P16 = 2, p <= 20: the second column block holds at most 4 real columns, 16..19): the two
// tiles of that block's row run on v_mfma_f64_4x4x4f64, which takes its operands in the 16x16x4
// lane layout with 4x4 block j on columns 4j..4j+3 (tools/mfma_layout.hip) and writes block j's
// D(m, n) to lane 16 m + 4 j + n -- exactly where the 16x16x4 tile keeps rows 0..3 of its D in
// acc[t][0].  Tile (1, 1): block 0 is columns 16..19 x 16..19; tile (1, 0): the A operand's first
// 4-lane group (columns 16..19) broadcast to all four groups gives columns 16..19 x 4j..4j+3 in
// block j.  16 MFMA cycles each instead of 64 (the LM Gram of configs[0], p = 20: 96 per k-step
// instead of 192); rows 4..15 of those tiles (columns 20..31: padding) are never formed.
template <int P16, bool T4 = false>
__device__ __forceinline__ void gram_kstep(d4 (&acc)[P16 * (P16 + 1) / 2], const double (&av)[P16],
                                           const double (&xv)[P16]) {
  if constexpr (T4) {
    static_assert(P16 == 2, "T4: two column blocks");
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], xv[0], acc[0], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(bcast_quad0(av[1]), xv[0], acc[1][0], 0, 0, 0);
    acc[2][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[1], xv[1], acc[2][0], 0, 0, 0);
  } else {
    int t = 0;
#pragma unroll
    for (int bi = 0; bi < P16; ++bi)
#pragma unroll
      for (int bj = 0; bj <= bi; ++bj, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[bi], xv[bj], acc[t], 0, 0, 0);
  }
}

// Poisson: per-row functions of the count y tabulated in LDS after the waves' images -- the initial
// pass's unit deviance at mu0 and lgamma(y + 1) with init_const behind them (PTAB: [2][POIS_TAB] + 8,
// rowmath.hpp poisson_init_table), the IRLS passes' y log y (YTAB: [POIS_TAB], poisson_ylogy_table,
// pass_row ylogy).  Filled by the whole workgroup (NTHREADS) before its first row.
template <int FAM, int LNK, bool PTAB, bool YTAB, int NTHREADS>
__device__ __forceinline__ void fill_poisson_tables(double* ptab, const PassArgs& a) {
  if constexpr (YTAB) {
    for (int k = threadIdx.x; k < POIS_TAB; k += NTHREADS) poisson_ylogy_table(ptab, k);
    __syncthreads();
  }
  if constexpr (PTAB) {
    for (int k = threadIdx.x; k < POIS_TAB; k += NTHREADS) poisson_init_table(ptab, a.mu0, k);
    if (threadIdx.x == 0) {
      const InitConst ic = init_const(FAM, link_of<LNK>(a.link), a.mode, a.mu0, link_by_link(FAM, LNK));
      for (int k = 0; k < 6; ++k) ptab[2 * POIS_TAB + k] = ic.v[k];
    }
    __syncthreads();
  }
}

// A k-step from a lane's operands: lane (rq, cl) takes x = X[row 4 s + rq, column 16 b + cl] from x(b) --
// an LDS read, a widened float or a stashed register -- and holds that row's w and w z.  The A operand
// is x w; X'Wz (and LMX: X'1 into x1, which is not touched otherwise) on the VALU.
template <bool T4, bool LMX, int P16, class X1, class XOf>
__device__ __forceinline__ void weighted_kstep(d4 (&acc)[P16 * (P16 + 1) / 2], double (&xz)[P16], X1&& x1, XOf&& x,
                                               double wr, double wzr) {
  double av[P16], xk[P16];
#pragma unroll
  for (int b = 0; b < P16; ++b) {
    xk[b] = x(b);
    av[b] = xk[b] * wr;
    xz[b] += xk[b] * wzr;
    if constexpr (LMX) x1[b] += xk[b];
  }
  gram_kstep<P16, T4>(acc, av, xk);
}

}  // namespace sglm
