// kernels.hpp -- host-side launchers of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace sglm {

// column-block count P16 of the fused kernel a pass over p columns runs (odd: K1r only)
int pass_variant(int p, int fused_split, int64_t ld);
int pass_stride(int P16);       // doubles per workgroup partial
int pass_wg_per_cu(int P16);    // workgroups per CU the variant is built for
bool pass_uses_split(int P16, int fused_split, int64_t ld);  // K1r (one 12-wave workgroup per CU) for this pass
// e0 / e1: HIP events the launch itself records at the kernel's start / end (hipExtLaunchKernel: no
// marker packets between the kernels of a pass; null = none)
hipError_t launch_pass(int P16, const PassArgs& a, int grid, hipStream_t st, hipEvent_t e0 = nullptr,
                       hipEvent_t e1 = nullptr);
hipError_t launch_pass_odd(int P16, const PassArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1);  // fused_odd.hip: K1r, P16 5..15 odd
hipError_t launch_stats(const StatsArgs& a, int grid, hipStream_t st);
// [nparts][NS] -> [NS]; host != null: also src[0, ncopy) (out inside it) into host memory the device can write
hipError_t launch_reduce_stats(const double* part, int nparts, double* out, hipStream_t st, const double* src = nullptr,
                               double* host = nullptr, int64_t ncopy = 0);
// LM.fit's solve on the device, bitwise the host Cholesky (p <= 64): beta[p], aux = {ybar, leave-Cholesky flag}.
// One pass (op.stats set; the Gram pass ran with PassArgs::lm_extras): also the residual statistics from
// the Gram pass's sums (x1 = X'1 [p] right after the packed Gram) into op.stats; with op.host the
// result buffer -- packed[0, ncopy) and beta / op.stats (which lie inside the same allocation past it,
// at the same offsets) -- is written to pinned host memory.
struct LmOnePass {
  const double* x1 = nullptr;
  double* stats = nullptr;  // [NS]: SSE, top, bot, rows, S_BAD = 1 when lm_drive must rerun the residual pass
  double* host = nullptr;
  int64_t ncopy = 0;
};
constexpr double LM_ONEPASS_MAX_RATIO = 1e4;  // max(y'y, b'X'Xb, n ybar^2) / min(SSE, top, bot) at most
hipError_t launch_lm_chol(const double* packed, int p, double ratio_min, double* beta, double* aux, hipStream_t st,
                          const LmOnePass& op = LmOnePass{});
// extra: elements past the NS scalars summed too (the LM Gram's X'1, narrow LMX), out[tri + p + NS + k]
hipError_t launch_reduce(const double* part, int64_t stride, int nparts, int p, int P16, double* out, hipStream_t st,
                         hipEvent_t e1 = nullptr, int extra = 0);
hipError_t launch_predict(const double* X, int64_t ld, int p, int64_t n, const double* beta, const double* off,
                          double* out, hipStream_t st, const ProcX& g);
hipError_t launch_unlink(double* v, const double* m, int64_t n, int family, int link, hipStream_t st);
hipError_t launch_ysum(const double* y, int64_t n, double* part, int nparts, hipStream_t st);
uint64_t splitmix64_host(uint64_t x);
hipError_t launch_synth(int kind, int64_t row0, int64_t n, int p, uint64_t seed, double scale, double* X, int64_t ld,
                        double* y, double* m, double* off, double* prior, hipStream_t st);

// narrow path (narrow.hip): p <= 64
int narrow_variant(int p);      // column blocks of 16 (1..4)
int narrow_stride(int P16);     // doubles per workgroup partial (reduce_partials_kernel layout)
int narrow_wg_per_cu();
int narrow_rows_per_wg(int P16); // rows one workgroup streams per block step (waves x rows per block)
hipError_t launch_narrow(int P16, const PassArgs& a, int grid, hipStream_t st, hipEvent_t e0 = nullptr,
                         hipEvent_t e1 = nullptr);

// per-row diagnostics (influence.hip): p <= 256
// workgroups of a mode (enum InflMode) over n rows; each owns the steps g, g + grid, ...: a fixed order
int infl_grid(int mode, int P16, int ncu, int64_t n);
// C (col-major p x p, symmetric) -> C~ in the kernels' operand order: the block triangle c <= b of
// 16 x 16 tiles (tile b (b + 1) / 2 + c), off-diagonal tiles doubled, zero past p; out [T][INFL_TILE]
void influence_tiles(const double* C, int p, double* out);
// One launcher for every mode, with grid = infl_grid of the same mode (e0 / e1 as launch_pass's):
//   INFL_ROWS    the diagnostics of the rows < n at a.beta (hat / resid / cooks; hpart [grid]: the sums of h)
//   INFL_QFORM   a.out = sqrt(max(0, dispersion q))
//   INFL_SCORE   the sandwich estimator's score weights into a.out (hat / resid / cooks / hpart unused)
//   INFL_USCORE  the signed scores u_i = w_i (y_i - mu_i) g'(mu_i) into a.out (need_q = 0: no MFMA product)
//   INFL_FIRTH   Firth's adjusted score: g* = sum_i (u_i + h_i r_i / 2) x_i, the sum of h and
//                (a.hat) h itself at a.beta against a.ct, into the partials a.gpart [grid][p + 1].  firth_is_fused:
//                one kernel and one read of X, else a.out [n] receives v and a second kernel streams X for X'v
//                (both between e0 and e1).
hipError_t launch_infl(int mode, int P16, const InflArgs& a, int grid, hipStream_t st, hipEvent_t e0 = nullptr,
                       hipEvent_t e1 = nullptr);
bool firth_is_fused(int P16);
// out [ncol] = the workgroups' partials part [nparts][ncol] added in a fixed order (hpart: one column; gpart: p + 1)
hipError_t launch_infl_sum(const double* part, int nparts, int ncol, double* out, hipStream_t st);

// multinomial logit (multinom.hip): p <= 256, 2 <= K <= MN_MAX_K, (K - 1) p <= MN_MAX_Q
// workgroups of the row kernel (and, per column block, of multinom_xtr_kernel) over n rows: a fixed order
int multinom_grid(int ncu, int64_t n);
// the score accumulates in the row kernel's own read of X at this shape (else R is stored and a second kernel reads X)
bool multinom_is_fused(int P16, int K);
// The rows at a.B in `mode` (enum MnMode) with grid = multinom_grid: the partials a.part [grid][a.stride].  MN_FULL
// past the fused shapes launches multinom_xtr_kernel behind the row kernel (e1 to e2; fused: e2 is not recorded).
hipError_t launch_multinom_rows(int mode, int P16, const MultinomArgs& a, int grid, hipStream_t st,
                                hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, hipEvent_t e2 = nullptr);
// out [ld] = pw pi_j sum_{l != j} pi_l (j == k) or pw pi_j pi_k of the rows < n, zeros on the padding rows
hipError_t launch_multinom_weight(const double* P, const double* prior, int64_t n, int64_t ld, int K, int j, int k,
                                  double* out, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// launch_infl_sum over partials `stride` doubles apart (ncol <= stride)
hipError_t launch_part_sum(const double* part, int nparts, int stride, int ncol, double* out, hipStream_t st);

// cluster sums (cluster.hip): the cluster-robust covariance's grouped scores
// segments of the n rows under `ids` (cluster_segments: maximal runs of one id, cut at every multiple
// of CLUSTER_TILE_ROWS): seg_start [nseg + 1], seg_cluster [nseg], either may be null; returns nseg,
// or -1 at an id outside [0, G)
int64_t cluster_segments(const int32_t* ids, int64_t n, int32_t G, int64_t* seg_start, int32_t* seg_cluster);
int cluster_sum_grid(int ncu, int64_t n, int p);
hipError_t launch_cluster_sum(const ClusterArgs& a, int grid, hipStream_t st, hipEvent_t e0 = nullptr,
                              hipEvent_t e1 = nullptr);
hipError_t launch_cluster_combine(const CombineArgs& a, int ncu, hipStream_t st, hipEvent_t e0 = nullptr,
                                  hipEvent_t e1 = nullptr);

// fixed-effects IRLS (fe.hip): per-row weights / scores and their per-segment sums, the effective offset,
// the fixed-effect update and the scaling of the group sums for the Gram pass over them
int fe_grid(int ncu, int64_t ntiles);
hipError_t launch_fe_weights(const SegRowArgs& a, int grid, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t launch_fe_offset(const FeOffsetArgs& a, int grid, hipStream_t st);
hipError_t launch_fe_alpha(const GroupArgs& a, hipStream_t st);
hipError_t launch_fe_scale(const GroupArgs& a, hipStream_t st);

// GEE fits (gee.hip): sqrt(w) / the scores and the four per-segment scalar sums, the moments of the group
// buffer (partials [grid][NS], then out [NS]: launch_reduce_stats' sums with M_NMAX replaced by the maximum),
// the scaling of the group sums for the Gram pass over them
constexpr int GEE_MOMENT_BLOCKS = 1024;  // at most; the grid is a function of G alone
int gee_moment_grid(int64_t G);
hipError_t launch_gee_rows(const SegRowArgs& a, int grid, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t launch_gee_moments(const GroupArgs& a, double* out, hipStream_t st);
hipError_t launch_gee_scale(const GroupArgs& a, hipStream_t st);

// two-way fixed effects (fe2.hip): the sums over factor 2's row lists, the gathers of the sweeps, the level
// update with its stop-rule maxima, the cross product S_X' Y, the offset and the effects
int fe2_grid(int ncu, int64_t units);
hipError_t launch_fe2_list_sum(const Fe2ListSumArgs& a, int ncu, hipStream_t st);
hipError_t launch_fe2_gather(const Fe2GatherArgs& a, int ncu, hipStream_t st);
hipError_t launch_fe2_update(const Fe2UpdateArgs& a, hipStream_t st);
hipError_t launch_fe2_cross(const Fe2CrossArgs& a, double* out, hipStream_t st);  // out [PR][PC]: the slices summed in order
hipError_t launch_fe2_offset(const Fe2OffsetArgs& a, hipStream_t st);
hipError_t launch_fe2_effect(const Fe2EffectArgs& a, hipStream_t st);
hipError_t launch_fe2_normalise(const Fe2NormArgs& a, hipStream_t st);
hipError_t launch_fe2_meat(const Fe2MeatArgs& a, hipStream_t st);

// theta terms of the negative binomial (theta.hip): [grid][NS] partials for launch_reduce_stats; loglik: T_LL too
hipError_t launch_theta_terms(const ThetaArgs& a, int grid, bool loglik, hipStream_t st, hipEvent_t e0 = nullptr,
                              hipEvent_t e1 = nullptr);

// wide path (wide.hip)
int wide_panels(int p);
int64_t wide_stride();
// ov: the overlapped-chunk variant (wide_rows_ov_kernel: <= 96 VGPRs, fits beside the Gram kernels)
hipError_t launch_wide_rows(const WideRowArgs& a, int grid, hipStream_t st, bool ov = false);
hipError_t launch_proc_gen(const ProcGenArgs& a, int grid, hipStream_t st);
int wide_gram_wg_per_cu(bool diag);
hipError_t launch_wide_gram(const WideGramArgs& a, bool diag, int grid, hipStream_t st);
hipError_t launch_wide_reduce(const double* part, int64_t stride, const int* st_range, int p, const double* rowpart,
                              int nrow, double* out, hipStream_t st);
hipError_t launch_sum_chunks(const double* chunks, int nch, int p, double* out, hipStream_t st);
hipError_t launch_unpack_lower(const double* packed, int p, double* A, double* b, hipStream_t st, bool full = false);
// x = A b, A column-major p x p, summed over k in ascending order (the reference's inv * b)
hipError_t launch_inv_gemv(const double* A, int p, const double* b, double* x, hipStream_t st);

}  // namespace sglm
