// multinom.hip -- the row stage of the multinomial logit fits (softmax regression) on a resident design with
// p <= 256, 2 <= K <= 16 classes and q = (K - 1) p <= 1024 (gfx950; multinom.cpp).
//
//   eta_0 = 0, eta_j = x' beta_j;  mx = max(0, eta_1, ...);  E_j = exp(eta_j - mx);  S = E_0 + E_1 + ...
//   pi_j = E_j / S for every j (pi_0 is never 1 - sum);  log pi_y = (eta_y - mx) - log S
//   R_ij = pw_i (1[y_i = j] - pi_ij), j = 1 .. K - 1;  the score g = vec(X'R)
//
// multinom_rows_kernel<P16, MODE, KM> is influence_body's register layout without its MFMA product: one wave owns
// 16 rows, lane (i, g) holds xv[c][s] = X[row i, column 16 c + 4 s + g], loaded straight from HBM (128 B contiguous
// per column), and the same registers serve the eta products and the score accumulators, as in firth_kernel.
//
// eta: VALU dot products against the padded B in LDS and one sum over the four lane groups per class -- not the
// transposed fp64 MFMA block column.  The MFMA form needs B as a 16-column tile whatever K is and its result in a
// d4 per column block beside xv; at K = 3 (the common case) that is 8x the flops for 2 used columns of 16, and
// the VALU form costs 4 P16 (K - 1) FMAs per lane and step, under the stream's time at every shape (K = 16:
// 15 / 4 FMA per byte of X).  By compiled register count the VALU form is also what leaves the accumulators
// their room: the row stage itself holds 8 P16 + ~40 VGPRs.
// After the group sum all four lanes of a row hold eta_j; each keeps it (then E_j) in an LDS slot of its own
// (slot[j][thread]: no lane reads another's, so no barrier), and the softmax runs redundantly on the four groups,
// which SIMD lanes idle otherwise -- every lane of a row then holds pi_j and R_j for its own columns.
//
// Modes: MN_DEV sums the scalars alone (sum pw log pi_y, sum pw, the rows whose y is no class code, the weighted
// class counts) and stores nothing per row; MN_FULL also stores P [K][ld] and forms the score.
// Score: with KM > 0 the lane accumulates R_j xv[c][s] in gacc[j][c][s] across the workgroup's steps (j unrolled to
// KM, guarded by j < K - 1; KM is the bucket 1, 2, 3, 4, 7 or 15 that holds K - 1), reduced at the end as
// firth_reduce does: 16 lanes, then the four waves through LDS, in a fixed order.  Where gacc does not fit beside
// xv (mn_fused below) the kernel stores R [K - 1][ld] and multinom_xtr_kernel streams X a second time: a lane
// per row, a wave per 4 columns and a workgroup per column block (blockIdx.y), all K - 1 classes' accumulators
// for its 4 columns in registers, into the same partials.
//
// Scalars: a Neumaier pair per lane (the counts: a pair per lane and class in LDS), then lanes, waves and
// (launch_part_sum) workgroups in a fixed order.  No floating-point atomics: two calls are bitwise equal.
//
// multinom_weight_kernel writes the Gram pass's row weights of one block pair of the Hessian from P:
// pw pi_j sum_{l != j} pi_l (no 1 - pi_j: nothing cancels as pi_j -> 1) or pw pi_j pi_k (the host negates).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rowmath.hpp"

namespace sglm {

namespace {

constexpr int MN_NW = 4;  // waves per workgroup
constexpr int MN_NT = 64 * MN_NW;
constexpr int MN_STEP = 16 * MN_NW;  // rows per workgroup step (multinom_xtr_kernel: a row per lane, the same 64)
constexpr int MN_WG_PER_CU = 2;

// The class buckets of the fused form: K - 1 <= KM.
constexpr int MN_NB = 6;
constexpr int MN_BUCKET[MN_NB] = {1, 2, 3, 4, 7, 15};
constexpr int mn_bucket(int km1) {
  for (int b = 0; b < MN_NB; ++b)
    if (km1 <= MN_BUCKET[b]) return b;
  return MN_NB - 1;
}
// Fused (the score in the row kernel's own read of X) while xv and gacc -- 8 P16 (KM + 1) VGPRs -- fit 256 VGPRs
// without scratch.  From the compiler's resource report at build time (-Rpass-analysis=kernel-resource-usage;
// VGPRs of the largest bucket without scratch per width, and the scratch bytes per lane of the next one):
//   P16   1: KM 15 229          2: KM 7 231 (15: 364 B)   3: KM 4 234 (7: 108 B)   4: KM 4 254 (7: 364 B)
//         5: KM 3 254 (4: 148 B)   6: KM 2 244 (3: 108 B)   7: KM 2 256 (3: 236 B)
//         8 / 9 / 10: KM 1 228 / 244 / 254 (2: 104 / 200 / 296 B)      11: KM 1 spills (44 B)
// -- every fitting pair has P16 (KM + 1) <= 21 and every spilling one >= 22.  (VGPR spills and scratch are 0 on the
// fitting side; the report also shows SGPR spills there -- 2 to 10 at P16 <= 3, 39 at P16 = 1, KM = 15: the guards
// j < K - 1 of the unrolled classes -- which go to VGPR lanes, not to scratch.)  The kernels without accumulators
// (MN_DEV, and MN_FULL storing R) take 104 .. 246 VGPRs and multinom_xtr_kernel 137, all without scratch.
constexpr int MN_FUSED_MAX = 21;
constexpr bool mn_fused(int P16, int KM) { return P16 * (KM + 1) <= MN_FUSED_MAX; }

__device__ __forceinline__ double mn_group_sum(double v) {  // over the four lane groups l / 16
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

__device__ __forceinline__ double mn_sum16(double t) {  // over the 16 lanes of a lane group
  t += __shfl_xor(t, 1);
  t += __shfl_xor(t, 2);
  t += __shfl_xor(t, 4);
  t += __shfl_xor(t, 8);
  return t;
}

template <int P16, int MODE, int KM>
__global__ void __launch_bounds__(MN_NT, MN_WG_PER_CU) multinom_rows_kernel(MultinomArgs a) {
  constexpr int W = 16 * P16;
  constexpr bool FULL = MODE == MN_FULL, GACC = KM > 0;
  static_assert(!GACC || FULL, "the score belongs to the full mode");
  // (K - 1) W <= q + 15 (K - 1)
  __shared__ double sB[MN_MAX_Q + 16 * (MN_MAX_K - 1)];
  __shared__ double slot[MN_MAX_K * MN_NT];  // eta_j, then E_j, of this lane's row; at the end the waves' score partials
  __shared__ double scnt[MN_MAX_K * 64 * 2];  // the class counts' Neumaier pairs of the 64 lanes with g = 0
  __shared__ double swave[MN_NW][3];
  static_assert(MN_NW * W <= MN_MAX_K * MN_NT, "the wave partials fit the slots");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int K = a.K, km1 = K - 1, p = a.p;
  for (int k = tid; k < km1 * W; k += MN_NT) {
    const int j = k / W, c = k - j * W;
    sB[k] = c < p ? a.B[j * p + c] : 0.0;
  }
  for (int k = tid; k < MN_MAX_K * 64 * 2; k += MN_NT) scnt[k] = 0.0;
  __syncthreads();
  double ll = 0.0, llc = 0.0, sw = 0.0, swc = 0.0, bad = 0.0;
  double gacc[GACC ? KM : 1][P16][4];
  if constexpr (GACC) {
#pragma unroll
    for (int j = 0; j < KM; ++j)
#pragma unroll
      for (int c = 0; c < P16; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) gacc[j][c][s] = 0.0;
  }
  const int64_t ld = a.ld;
  const int64_t nsteps = (a.n + MN_STEP - 1) / MN_STEP;
  for (int64_t step = blockIdx.x; step < nsteps; step += gridDim.x) {
    const int64_t row = step * MN_STEP + (int64_t)(wave * 16 + i);
    const bool live = row < a.n;
    // Unconditional loads from clamped addresses, as influence_body's: a row >= n reads row n - 1 (its weight is 0
    // and nothing of it is stored), a column >= p reads column p - 1 and meets the zeros of the padded B (the
    // fused score's accumulators of those columns are never stored).
    const int64_t rr = live ? row : a.n - 1;
    double xv[P16][4];
    {
      const double* xp = a.X + rr + (int64_t)g * ld;
      const int64_t ld4 = 4 * ld;
#pragma unroll
      for (int c = 0; c < P16 - 1; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          xv[c][s] = *xp;
          xp += ld4;
        }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int col = min(16 * (P16 - 1) + 4 * s + g, p - 1);
        xv[P16 - 1][s] = a.X[rr + (int64_t)col * ld];
      }
    }
    const double pw = live ? (a.prior ? a.prior[rr] : 1.0) : 0.0;
    // a row of weight 0 contributes nothing and its y is not looked at
    int yc = 0;
    double pwe = 0.0;
    if (pw > 0.0) {
      const double yv = a.y[rr];
      const bool in = yv >= 0.0 && yv < (double)K;
      yc = in ? (int)yv : 0;
      if (in && yv == (double)yc) {
        pwe = pw;
      } else {
        yc = 0;
        if (g == 0) bad += 1.0;
      }
    }
    double mx = 0.0;
    for (int j = 0; j < km1; ++j) {
      const double* bj = sB + j * W + g;
      double e = 0.0;
#pragma unroll
      for (int c = 0; c < P16; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) e = fma(xv[c][s], bj[16 * c + 4 * s], e);
      e = mn_group_sum(e);
      slot[(j + 1) * MN_NT + tid] = e;
      mx = fmax(mx, e);
    }
    const double eta_y = yc == 0 ? 0.0 : slot[yc * MN_NT + tid];
    double S = exp(-mx);
    slot[tid] = S;
    for (int j = 1; j < K; ++j) {
      const double E = exp(slot[j * MN_NT + tid] - mx);
      slot[j * MN_NT + tid] = E;
      S += E;
    }
    if (g == 0 && pwe > 0.0) {
      neumaier_add(ll, llc, pwe * ((eta_y - mx) - log(S)));
      neumaier_add(sw, swc, pwe);
      double* cp = scnt + (yc * 64 + wave * 16 + i) * 2;
      double cs = cp[0], cc = cp[1];
      neumaier_add(cs, cc, pwe);
      cp[0] = cs;
      cp[1] = cc;
    }
    if constexpr (FULL) {
      const bool store = g == 0 && live;
      if (store) a.P[rr] = slot[tid] / S;
      if constexpr (GACC) {
#pragma unroll
        for (int j = 0; j < KM; ++j)
          if (j < km1) {
            const double pi = slot[(j + 1) * MN_NT + tid] / S;
            if (store) a.P[(int64_t)(j + 1) * ld + rr] = pi;
            const double r = pwe == 0.0 ? 0.0 : pwe * ((yc == j + 1 ? 1.0 : 0.0) - pi);
#pragma unroll
            for (int c = 0; c < P16; ++c)
#pragma unroll
              for (int s = 0; s < 4; ++s) gacc[j][c][s] = fma(r, xv[c][s], gacc[j][c][s]);
          }
      } else {
        for (int j = 1; j < K; ++j) {
          const double pi = slot[j * MN_NT + tid] / S;
          if (store) {
            a.P[(int64_t)j * ld + rr] = pi;
            a.R[(int64_t)(j - 1) * ld + rr] = pwe == 0.0 ? 0.0 : pwe * ((yc == j ? 1.0 : 0.0) - pi);
          }
        }
      }
    }
  }
  // the workgroup's partial: the score (fused), then the scalars -- lanes, then waves, in a fixed order
  double* part = a.part + (int64_t)blockIdx.x * a.stride;
  double* sc = part + a.nscore;
  ll = mn_sum16(ll + llc);  // (the lanes of the groups 1 .. 3 hold zeros)
  sw = mn_sum16(sw + swc);
  bad = mn_sum16(bad);
  if (lane == 0) {
    swave[wave][MN_LL] = ll;
    swave[wave][MN_SUMW] = sw;
    swave[wave][MN_BAD] = bad;
  }
  __syncthreads();  // swave and scnt are complete; every wave is done with its slots
  if (tid < 3) {
    double s = swave[0][tid];
    for (int k = 1; k < MN_NW; ++k) s += swave[k][tid];
    sc[tid] = s;
  }
  if (tid >= 64 && tid < 64 + MN_MAX_K) {
    const int k = tid - 64;
    double s = 0.0, c = 0.0;
    for (int t = 0; t < 64; ++t) {
      neumaier_add(s, c, scnt[(k * 64 + t) * 2]);
      c += scnt[(k * 64 + t) * 2 + 1];
    }
    sc[MN_COUNT + k] = s + c;
  }
  if constexpr (GACC) {
    double* red = slot;  // [MN_NW][W]
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < km1) {
        __syncthreads();  // the previous class's partials are read
#pragma unroll
        for (int c = 0; c < P16; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double t = mn_sum16(gacc[j][c][s]);
            if (i == 0) red[wave * W + 16 * c + 4 * s + g] = t;
          }
        __syncthreads();
        for (int col = tid; col < p; col += MN_NT) {
          double t = red[col];
          for (int k = 1; k < MN_NW; ++k) t += red[k * W + col];
          part[j * p + col] = t;
        }
      }
  }
}

// X'R of the stored R, the shapes past the fused ones: a second stream of X over the row kernel's steps and
// grid.x, into the first (K - 1) p entries of the same partials.  A lane is a row (512 contiguous bytes per column
// and wave), wave w of workgroup (., b) owns the columns 16 b + 4 w .. + 3 and carries one accumulator per class and
// column across the steps (the classes unrolled to 15, guarded by j < K - 1); at the end each is summed over the
// 64 lanes in a fixed order.  R is re-read once per column block: (K - 1) / 16 of X's bytes.
__global__ void __launch_bounds__(MN_NT, MN_WG_PER_CU) multinom_xtr_kernel(MultinomArgs a) {
  constexpr int KM = MN_MAX_K - 1;
  const int lane = threadIdx.x & 63;
  const int col0 = 16 * (int)blockIdx.y + 4 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int km1 = a.K - 1, p = a.p;
  if (col0 >= p) return;  // (no barrier below)
  double acc[KM][4];
#pragma unroll
  for (int j = 0; j < KM; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[j][k] = 0.0;
  const int64_t ld = a.ld;
  const int64_t nsteps = (a.n + MN_STEP - 1) / MN_STEP;
  for (int64_t step = blockIdx.x; step < nsteps; step += gridDim.x) {
    const int64_t row = step * MN_STEP + lane;
    const bool live = row < a.n;
    const int64_t rr = live ? row : a.n - 1;  // clamped: r, not x, is masked
    double x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = a.X[rr + (int64_t)min(col0 + k, p - 1) * ld];  // a column >= p: never stored
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < km1) {
        const double r = live ? a.R[(int64_t)j * ld + rr] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[j][k] = fma(r, x[k], acc[j][k]);
      }
  }
  double* part = a.part + (int64_t)blockIdx.x * a.stride;
#pragma unroll
  for (int j = 0; j < KM; ++j)
    if (j < km1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double t = mn_sum16(acc[j][k]);
        t += __shfl_xor(t, 16);
        t += __shfl_xor(t, 32);
        if (lane == 0 && col0 + k < p) part[j * p + col0 + k] = t;
      }
    }
}

__global__ void __launch_bounds__(256) multinom_weight_kernel(const double* __restrict__ P,
                                                              const double* __restrict__ prior, int64_t n, int64_t ld,
                                                              int K, int j, int k, double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= ld) return;
  double w = 0.0;
  if (r < n) {
    const double pw = prior ? prior[r] : 1.0;
    double f;
    if (j == k) {
      f = 0.0;  // 1 - pi_j as the sum of the other classes' probabilities, baseline included
      for (int l = 0; l < K; ++l)
        if (l != j) f += P[(int64_t)l * ld + r];
    } else {
      f = P[(int64_t)k * ld + r];
    }
    w = pw == 0.0 ? 0.0 : pw * (P[(int64_t)j * ld + r] * f);
  }
  out[r] = w;
}

// The kernels of one width; fused[b]: null where the bucket's accumulators do not fit (not built)
typedef void (*MnKernel)(MultinomArgs);
struct MnWidth {
  MnKernel dev, full, fused[MN_NB];
};
template <int N, int B>
MnKernel mn_fused_kernel() {
  if constexpr (mn_fused(N, MN_BUCKET[B])) return multinom_rows_kernel<N, MN_FULL, MN_BUCKET[B]>;
  else return nullptr;
}
template <int N>
MnWidth mn_width() {
  return MnWidth{multinom_rows_kernel<N, MN_DEV, 0>,
                 multinom_rows_kernel<N, MN_FULL, 0>,
                 {mn_fused_kernel<N, 0>(), mn_fused_kernel<N, 1>(), mn_fused_kernel<N, 2>(), mn_fused_kernel<N, 3>(),
                  mn_fused_kernel<N, 4>(), mn_fused_kernel<N, 5>()}};
}

const MnWidth* mn_kernels(int P16) {
#define K(N) mn_width<N>()
  static const MnWidth all[MAX_P16] = {K(1), K(2),  K(3),  K(4),  K(5),  K(6),  K(7),  K(8),
                                       K(9), K(10), K(11), K(12), K(13), K(14), K(15), K(16)};
#undef K
  return P16 >= 1 && P16 <= MAX_P16 ? &all[P16 - 1] : nullptr;
}

}  // namespace

// One workgroup per resident slot, two per CU: the grid -- and with it the order of every sum -- depends on the
// shape and the device only.  multinom_xtr_kernel takes the same grid.x: it fills the row kernel's partials.
int multinom_grid(int ncu, int64_t n) {
  const int64_t steps = std::min<int64_t>((n + MN_STEP - 1) / MN_STEP, (int64_t)1 << 30);
  return std::max(1, (int)std::min<int64_t>(steps, (int64_t)ncu * MN_WG_PER_CU));
}

bool multinom_is_fused(int P16, int K) {
  return K >= 2 && K <= MN_MAX_K && mn_fused(P16, MN_BUCKET[mn_bucket(K - 1)]);
}

hipError_t launch_multinom_rows(int mode, int P16, const MultinomArgs& a, int grid, hipStream_t st, hipEvent_t e0,
                                hipEvent_t e1, hipEvent_t e2) {
  const MnWidth* w = mn_kernels(P16);
  if (!w || a.K < 2 || a.K > MN_MAX_K || (a.K - 1) * a.p > MN_MAX_Q) return hipErrorInvalidValue;
  const dim3 b(MN_NT);
  if (mode == MN_DEV) {
    hipExtLaunchKernelGGL(w->dev, dim3(grid), b, 0, st, e0, e1, 0, a);
  } else if (multinom_is_fused(P16, a.K)) {
    hipExtLaunchKernelGGL(w->fused[mn_bucket(a.K - 1)], dim3(grid), b, 0, st, e0, e1, 0, a);
  } else {
    hipExtLaunchKernelGGL(w->full, dim3(grid), b, 0, st, e0, e1, 0, a);
    hipExtLaunchKernelGGL(multinom_xtr_kernel, dim3(grid, P16), b, 0, st, nullptr, e2, 0, a);
  }
  return hipGetLastError();
}

hipError_t launch_multinom_weight(const double* P, const double* prior, int64_t n, int64_t ld, int K, int j, int k,
                                  double* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if (ld <= 0) return hipSuccess;
  hipExtLaunchKernelGGL(multinom_weight_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, st, e0, e1, 0, P,
                        prior, n, ld, K, j, k, out);
  return hipGetLastError();
}

}  // namespace sglm
