// common.hpp -- shared definitions for the sparkGLM MI355X engine (host + device).
#pragma once
#include <cstdint>

namespace sglm {

// Rows per LDS row block of the fused pass (one DMA'd tile of X).
constexpr int RB = 32;
// Scalar slots appended to every packed partial / reduced buffer.
constexpr int NS = 8;
enum Scalar : int { S_DEV = 0, S_PEARSON = 1, S_LL = 2, S_BAD = 3, S_AUX0 = 4, S_AUX1 = 5, S_AUX2 = 6, S_SUMW = 7 };

// Pass modes (shared with sglm_backend.pass in include/sglm.h).
enum PassMode : int {
  MODE_IRLS = 0,        // eta = X beta + offset (etaCreate, GLM.scala:321-332)
  MODE_INIT_SINGLE = 1, // eta = link(mu0, m), mu = mu0            (GLM.scala:263-270)
  MODE_INIT_MULTI = 2,  // eta = link(mu0, m), mu = unlink(eta, m) (GLM.scala:429-442, 370)
  MODE_LM_GRAM = 3,     // w = 1, z = y: X'X and X'y (LM.scala:142-155)
  MODE_LM_RESID = 4     // no Gram: SSE/SSR/SST at beta (LM.scala:160-188)
};

enum Family : int { FAM_BINOMIAL = 0, FAM_GAUSSIAN = 1, FAM_POISSON = 2, FAM_GAMMA = 3, FAM_NEGBIN = 4 };
enum Link : int {
  LNK_LOGIT = 0, LNK_PROBIT = 1, LNK_CLOGLOG = 2, LNK_IDENTITY = 3, LNK_LOG = 4, LNK_INVERSE = 5, LNK_SQRT = 6
};
// Link template argument of the per-family instantiations that read the link from their arguments at
// run time (PassArgs::link ...) and take the out-of-line reference row functions for every row.
constexpr int LNK_RT = -1;

// The (family, link) pairs of the engine (R's family objects: three links per family; the negative
// binomial's are MASS::negative.binomial's).
constexpr bool family_link_pair(int fam, int lnk) {
  return (fam == FAM_BINOMIAL && (lnk == LNK_LOGIT || lnk == LNK_PROBIT || lnk == LNK_CLOGLOG)) ||
         (fam == FAM_GAUSSIAN && (lnk == LNK_IDENTITY || lnk == LNK_LOG || lnk == LNK_INVERSE)) ||
         (fam == FAM_POISSON && (lnk == LNK_LOG || lnk == LNK_IDENTITY || lnk == LNK_SQRT)) ||
         (fam == FAM_GAMMA && (lnk == LNK_INVERSE || lnk == LNK_IDENTITY || lnk == LNK_LOG)) ||
         (fam == FAM_NEGBIN && (lnk == LNK_LOG || lnk == LNK_SQRT || lnk == LNK_IDENTITY));
}
// The non-canonical pairs of the extension families: the only ones whose mu = unlink(eta) can leave the
// family's range (R's validmu / valideta), which the row functions report as a NaN unit deviance
// (rowmath.hpp link_row_valid) and the drivers as SGLM_EINVAL.  None of the negative binomial's links is
// its canonical one (log(mu / (mu + theta))), so all three of its pairs are in this set.
constexpr bool noncanonical_pair(int fam, int lnk) {
  return family_link_pair(fam, lnk) && fam != FAM_BINOMIAL &&
         !((fam == FAM_GAUSSIAN && lnk == LNK_IDENTITY) || (fam == FAM_POISSON && lnk == LNK_LOG) ||
           (fam == FAM_GAMMA && lnk == LNK_INVERSE));
}

// The one dispatch of a run-time (family, link) onto the kernels' compile-time <FAM, LNK> instantiations
// (every launcher goes through it): a dedicated instantiation for the binomial links, the three canonical
// pairs, gamma / log and negative binomial / log; the other pairs run their family's LNK_RT instantiation.  f(Fam, Lnk) receives
// the pair as std::integral_constant-like tags; false: the pair has no instantiation (the launcher returns
// hipErrorInvalidValue -- it never runs another link's kernel).
template <int V>
struct IntTag {
  static constexpr int value = V;
};
template <class F>
inline bool dispatch_family_link(int fam, int lnk, F&& f) {
  if (!family_link_pair(fam, lnk)) return false;
  if (fam == FAM_BINOMIAL) {
    if (lnk == LNK_LOGIT) f(IntTag<FAM_BINOMIAL>{}, IntTag<LNK_LOGIT>{});
    else if (lnk == LNK_PROBIT) f(IntTag<FAM_BINOMIAL>{}, IntTag<LNK_PROBIT>{});
    else f(IntTag<FAM_BINOMIAL>{}, IntTag<LNK_CLOGLOG>{});
  } else if (fam == FAM_GAUSSIAN) {
    if (lnk == LNK_IDENTITY) f(IntTag<FAM_GAUSSIAN>{}, IntTag<LNK_IDENTITY>{});
    else f(IntTag<FAM_GAUSSIAN>{}, IntTag<LNK_RT>{});
  } else if (fam == FAM_POISSON) {
    if (lnk == LNK_LOG) f(IntTag<FAM_POISSON>{}, IntTag<LNK_LOG>{});
    else f(IntTag<FAM_POISSON>{}, IntTag<LNK_RT>{});
  } else if (fam == FAM_GAMMA) {
    if (lnk == LNK_INVERSE) f(IntTag<FAM_GAMMA>{}, IntTag<LNK_INVERSE>{});
    else if (lnk == LNK_LOG) f(IntTag<FAM_GAMMA>{}, IntTag<LNK_LOG>{});
    else f(IntTag<FAM_GAMMA>{}, IntTag<LNK_RT>{});
  } else {
    if (lnk == LNK_LOG) f(IntTag<FAM_NEGBIN>{}, IntTag<LNK_LOG>{});
    else f(IntTag<FAM_NEGBIN>{}, IntTag<LNK_RT>{});
  }
  return true;
}
// the link slot of the instantiation dispatch_family_link picks (LNK_RT or the link itself)
constexpr int dispatched_link(int fam, int lnk) {
  return (noncanonical_pair(fam, lnk) && !((fam == FAM_GAMMA || fam == FAM_NEGBIN) && lnk == LNK_LOG)) ? LNK_RT : lnk;
}

// Which families carry their final statistics in the narrow pass (PassArgs::stats_in_pass;
// rowmath.hpp pass_row_stats): binomial / logit (without m), Poisson / log, Gamma / inverse.
constexpr bool stats_in_pass_family(int fam, int lnk) {
  return (fam == FAM_BINOMIAL && lnk == LNK_LOGIT) || (fam == FAM_POISSON && lnk == LNK_LOG) ||
         (fam == FAM_GAMMA && lnk == LNK_INVERSE);
}

// Cache policy of the design-streaming LDS-DMA (global_load_lds aux): non-temporal.  Every byte of X
// is read once per pass, so it should not displace what the caches hold (round 5, same box: 1B x 32
// logit pass 45.92 -> 44.84 ms, 200M x 32 -1.0 %, 125M x 64 Poisson -0.4 %, 30M x 256 -0.6 %,
// bitwise the default policy).  The wide path's panels are re-read by several super-tiles: default there.
constexpr int DMA_NT = 2;

// Largest column-block count of the fused (single-panel) kernel: p <= 16*16 = 256.
constexpr int MAX_P16 = 16;

inline int64_t tri_count(int64_t p) { return p * (p + 1) / 2; }
inline int64_t packed_len(int64_t p) { return tri_count(p) + p + NS; }

// Arguments of one fused pass launch.
struct PassArgs {
  const double* X;      // col-major, leading dimension ld, 4*nq columns (zero past p)
  int64_t ld;
  int p;
  int nq;               // column quads stored: ceil(p / 4)
  const double* y;
  const double* m;      // may be null (binomial trials = 1)
  const double* off;    // may be null
  const double* prior;  // may be null
  const double* beta;   // device, >= p entries (MODE_IRLS / MODE_LM_RESID)
  int64_t n;            // valid rows
  int64_t nblocks;      // row blocks of RB rows (ld == nblocks*RB)
  int family, link, mode;
  double mu0;           // init modes
  double ybar;          // LM resid mode
  double* partials;     // [grid][stride]
  int64_t stride;
  double* eta_out;      // optional [n]: eta of MODE_IRLS rows (for the final statistics)
  int stats_in_pass;    // narrow binomial/logit IRLS pass without m: pearson / loglik / bad in the
                        // pass's scalars instead of the eta store + stats_kernel
  int no_gram;          // deviance-only pass (glm_drive's speculative last pass): row stage, no Gram
  int fused_split;      // split-role kernel K1r (irls_pass_r_kernel) from P16 >= threshold: 1 default, 0 never, N: P16 >= N
  int lm_extras;        // narrow LM Gram pass of the one-round-trip LM.fit: X'1 after the scalars, y'y in S_PEARSON
  double theta;         // FAM_NEGBIN: the dispersion parameter (sglm_set_theta); last, so every other field keeps its offset
};

// ---- wide-design path (p > 16*MAX_P16): row kernel + panel-pair Gram kernel ----
constexpr int WIDE_PANEL = 128;  // columns per Gram panel (8 tile blocks of 16)
constexpr int MAX_P_WIDE = 8192;

// Procedural design (sglm_synth_procedural): X is regenerated in the kernels, never stored.
struct ProcX {
  int on;               // 0: X is the resident image
  int kind, p;
  int64_t row0, n;      // global row of local row 0; valid rows
  uint64_t kx;          // splitmix64(seed)
  double scale;         // 1/sqrt(p)
};

struct WideRowArgs {
  const double* X;
  int64_t ld;
  int p;
  const double* y;
  const double* m;
  const double* off;
  const double* prior;
  const double* beta;   // device [p] (MODE_IRLS)
  int64_t n, n_pad;
  int family, link, mode;
  double mu0, ybar;
  double* w;            // [n_pad] working weights (0 on padding rows)
  double* wz;           // [n_pad] w * z
  double* eta_out;      // optional [n]
  double* row_partials; // [grid][NS]
  ProcX proc;
  int64_t r_begin, r_end;  // rows [r_begin, r_end) of this launch (multiples of 4; r_end may pass n_pad)
  double* xs_out;       // procedural chunks: the generated X rows stored here (column-major,
  int64_t xs_ld;        //   leading dimension xs_ld, local row = row - r_begin), else null
  const double* eta_in; // procedural chunks after proc_gen_kernel: X beta of rows < n (MODE_IRLS), else null
  double theta;         // FAM_NEGBIN: the dispersion parameter (last: the other fields keep their offsets)
};

// Procedural chunks: the lean generator (wide.hip proc_gen_kernel) -- X rows [r_begin, r_end) into
// the scratch and X beta (no offset) of the rows < proc.n into eta_raw.
struct ProcGenArgs {
  ProcX proc;
  const double* beta;   // device [p], or null (no eta: the initial pass)
  double* xs;           // scratch, column-major, leading dimension xs_ld, local row = row - r_begin
  int64_t xs_ld;
  int64_t r_begin, r_end;
  double* eta_raw;      // [n], global row index
};

// One run of 16-row blocks of one super-tile, processed by one workgroup of the persistent
// Gram kernel and written to partial slot `slot`: blocks b0, b0 + bs, b0 + 2 bs, ... < b1
// (bs = 1: consecutive blocks; bs = k: the k workgroups of a super-tile interleave block by
// block, so every workgroup of the launch sweeps the same rows at the same time).
struct WidePiece {
  int64_t b0, b1;       // blocks of WIDE_RB rows
  int st;               // super-tile I(I+1)/2 + J
  int slot;             // partial slot (slots of one super-tile are consecutive)
  int64_t bs;           // block stride
};
constexpr int WIDE_RB = 16;   // rows per Gram-kernel LDS block

struct WideGramArgs {
  const double* X;
  int64_t ld;
  int ncols;            // columns stored (multiple of 8, zero past p)
  const double* w;
  const double* wz;
  const WidePiece* pieces;
  const int* wg_begin;  // [grid + 1]: pieces of workgroup g are [wg_begin[g], wg_begin[g+1])
  double* partials;     // [slots][stride]
  int64_t stride;
  ProcX proc;
  int64_t nb_lim;       // blocks of this launch's rows: pieces are clipped to [b0, min(b1, nb_lim))
};

// Row quadratic forms q_i = x_i' C x_i and the per-row diagnostics built on them (influence.hip).
constexpr int INFL_TILE = 256;  // doubles per 16 x 16 tile of C~ (MFMA operand order, influence_tiles)
// what the kernel does with a row: the diagnostics at beta, sqrt(phi q) alone, the sandwich
// estimator's score weight omega = u^2 / (1 - h)^k, the signed score u itself,
// the factor of the cluster sums (cluster.hip), or Firth's adjusted score
enum InflMode : int { INFL_ROWS = 0, INFL_QFORM = 1, INFL_SCORE = 2, INFL_USCORE = 3, INFL_FIRTH = 4 };
struct InflArgs {
  const double* X;      // col-major, leading dimension ld; columns >= p are never read
  int64_t ld;
  int p;
  int64_t n;            // rows; rows >= n are never read or stored
  const double* ct;     // C~ tiles [P16 (P16 + 1) / 2][INFL_TILE] (null with need_q = 0)
  int need_q;           // 0: no MFMA product (residuals only)
  // influence_kernel: the row stage at beta
  const double* beta;   // device [p]
  const double* y;
  const double* m;      // may be null
  const double* off;    // may be null
  const double* prior;  // may be null
  int family, link, resid_type;
  // score_kernel: omega = u^2 / (1 - h)^hc_k, u = w (y - mu) g'(mu), h = w q (hc_k = 0: need_q = 0).
  // (In the alignment gap before dispersion: the argument block of the other two kernels keeps its layout.)
  int hc_k;
  double dispersion;    // phi of Cook's distance / of the qform_kernel's sqrt(phi q)
  double* hat;          // outputs [n], any may be null
  double* resid;
  double* cooks;
  double* hpart;        // [grid] per-workgroup sums of h (null: not wanted)
  // qform_kernel: out[i] = sqrt(max(0, dispersion * q_i)); score_kernel: out[i] = omega_i
  double* out;
  // FAM_NEGBIN: the dispersion parameter.  hc_k took the block's only 4-byte gap and a double needs 8, so
  // theta goes last: every other field keeps its offset.
  double theta;
  // firth_kernel: per-workgroup partials [grid][p + 1] of the adjusted score and, last, the sum of h; past the
  // fused widths out [n] receives v for firth_xtv_kernel.  After theta: every other field keeps its offset.
  double* gpart;
};

// Cluster sums S[g, :] = sum_{i: id_i = g} u_i x_i (cluster.hip).  A segment is a
// maximal run of consecutive rows with one id, cut at every multiple of CLUSTER_TILE_ROWS.
constexpr int CLUSTER_TILE_ROWS = 128;
struct ClusterArgs {
  const double* X;           // col-major, leading dimension ld (a multiple of 32, rows >= n zero)
  int64_t ld;
  int p;
  int64_t n;
  const double* u;           // [ld] signed scores, zero on the rows >= n
  const int64_t* seg_start;  // [nseg + 2]: first row of each segment, n, and a sentinel past every row
  const int64_t* tile_seg;   // [ntiles + 1]: first segment of each row tile
  int64_t ntiles;
  double* R;                 // [nseg][p] segment sums
};
// One level of the combine: chunk k sums the rows in[idx[q]] (idx null: in[q]), q in [chunk_start[k],
// chunk_start[k + 1]), in that order, into S[g, :] (chunk_dst[k] = g >= 0: the whole of cluster g) or
// into row -(chunk_dst[k] + 1) of out (one of several chunks of a cluster: the next level's input).
struct CombineArgs {
  const double* in;          // rows of p doubles
  const int64_t* idx;
  const int64_t* chunk_start;  // [nchunk + 1]
  const int64_t* chunk_dst;    // [nchunk]
  int64_t nchunk;
  int p;
  double* S;                 // col-major G x p, leading dimension ldS
  int64_t ldS;
  double* out;
};
constexpr int CLUSTER_CHUNK = 64;  // rows one thread of the combine adds

// The steps over the cluster factor: fixed-effects (within) IRLS (fe.hip; fe.cpp) and GEE with
// an exchangeable working correlation (gee.hip; gee.cpp; K13).  Their row kernels share one tiling and one
// argument block (segrows.hpp): one streaming read of the row vectors (never X), one value per row into `w` and
// NQ sums per segment into Q [nseg][NQ], by kind.
// fe_weights_kernel, NQ = 2:
//   FE_WZ     w_i (the working weight) | sum w z, sum w     at eta (mode MODE_IRLS) or at mu0 (the init modes)
//   FE_SCORE  u_i (the signed score)   | sum u,   0
//   FE_CHECK  nothing                  | sum y,   sum (m - y)  (binomial; else the row count) over the rows of
//                                        positive prior weight: the uninformative-group check
// gee_rows_kernel, NQ = GEE_NQ: sum d z | rows of positive prior weight | sum e | sum e^2 --
//   GEE_STEP   d_i = sqrt(w_i)                    at eta (mode MODE_IRLS) or at mu0 (the init modes)
//   GEE_SCORE  d_i e_i = w_i (y_i - mu_i) g'(mu_i)  (the four sums are GEE_STEP's)
//   GEE_COUNT  nothing; only the row counts are summed (no eta is read): the refusals before the first pass
// e_i = d_i (y_i - mu_i) g'(mu_i), z_i the working response without the offset (rowmath.hpp working_wz).
enum FeKind : int { FE_WZ = 0, FE_SCORE = 1, FE_CHECK = 2 };
enum GeeKind : int { GEE_STEP = 0, GEE_SCORE = 1, GEE_COUNT = 2 };
constexpr int GEE_NQ = 4;
struct SegRowArgs {
  const double* y;
  const double* eta;         // eta of the last pass (offset included); not read in the init modes
  const double* m;           // may be null
  const double* off;         // FE: the effective offset o* = o + alpha_g; GEE: the rows' own, may be null
  const double* prior;       // may be null
  int64_t n, ld;             // rows; w is written up to ld (zeros past n)
  int family, link, mode, kind;
  double mu0, theta;
  const int64_t* seg_start;  // the segments of sglm_set_clusters (ClusterArgs)
  const int64_t* tile_seg;
  int64_t ntiles;
  double* w;                 // [ld]; null: not stored (FE_CHECK, GEE_COUNT)
  double* Q;                 // [nseg][NQ]
  // fe_weights_kernel: the two values Q sums, per row [ld] (zeros past n and on rows of prior weight 0); null:
  // not stored.  va: w z | u | y; vb: w | 0 | m - y or 1.  The two-way fits sum them over factor 2's row lists.
  double* va;
  double* vb;
};
// fe_offset_kernel: out_i = off_i + alpha[cluster of row i] per segment, zeros on the rows in [n, ld)
struct FeOffsetArgs {
  const double* off;         // may be null
  const double* alpha;       // [G]
  const int64_t* seg_start;
  const int64_t* tile_seg;
  const int64_t* seg_cluster;  // [nseg]
  int64_t ntiles, n, ld;
  double* out;               // [ld]
};
// The group sums as one buffer (one all-reduce), ld = G rounded up to 32, col-major: FE S [ld x p] | t | W; GEE
// s [ld x p] | t | n | E | Q.  The kernels over its G rows share one argument block.
// fe_alpha_kernel: alpha_g += (t_g - s_g' beta) / W_g where W_g > 0.
// fe_scale_kernel: the design X [ld x p] and response y [ld] of the Gram pass over the groups --
//   meat = 0: x_g = s_g / sqrt(W_g), y_g = t_g / sqrt(W_g)        (X'X = sum s s' / W, X'y = sum s t / W)
//   meat = 1: x_g = S_g - U_g s_g / W_g, y_g = 0; S | U from `grp`, s | W from `grp2`
// rows with W_g = 0 (or not > 0): exact zeros.
// gee_moments_kernel: per-block partials [grid][NS] of GeeMoment over the G rows (M_NMAX a maximum).
// gee_scale_kernel: c_g = rho / (1 - rho + n_g rho); X and y of the Gram pass --
//   meat = 0: x_g = sqrt(|c_g|) s_g, y_g = sqrt(|c_g|) t_g       (sign(c_g) = sign(rho): applied on the host)
//   meat = 1: x_g = (S1_g - c_g E_g s_g) / (1 - rho), y_g = 0; S1 from `grp`, s | n | E from `grp2`
// rows with n_g = 0: exact zeros.
enum GeeMoment : int { M_E2 = 0, M_Q = 1, M_PAIRS = 2, M_N = 3, M_NMAX = 4, M_GEFF = 5, GEE_NM = 6 };
struct GroupArgs {
  const double* grp;
  const double* grp2;        // the step's own sums beside the score-weighted ones in grp (the scale kernels)
  int64_t G, ld;
  int p, meat;
  double rho;                // gee_scale_kernel
  const double* beta;        // device [p] (fe_alpha_kernel)
  double* alpha;             // [G] (fe_alpha_kernel)
  double* X;
  double* y;
  double* partials;          // gee_moments_kernel: [grid][NS]
};

// Two-way fixed effects: a second absorbed factor beside the cluster factor (fe2.hip; fe2.cpp).
// Factor 2's rows are listed per level in ascending order (a stable counting sort by code) and each level's
// list is cut into chunks of FE2_CHUNK positions; the chunks, already ordered by level, feed combine_kernel.
constexpr int FE2_CHUNK = 128;
// The per-row values it sums (w z and w; y and m - y for the check) are fe_weights_kernel's (SegRowArgs::va, vb).
// fe2_list_sum_kernel: R[k, j] = sum_{q in chunk k} v[row] X[row, j] (j < p), r0[row] (j = p), r1[row]
// (j = p + 1), row = list[q], positions in ascending order.  p = 0: only the two row vectors are summed.
struct Fe2ListSumArgs {
  const double* X;           // col-major, leading dimension ld
  int64_t ld;
  int p;
  const double* v;
  const double* r0;
  const double* r1;
  const int64_t* list;       // [n] rows ordered by factor-2 level, ascending within a level
  const int64_t* chunk_start;  // [nchunk + 1] positions in list
  int64_t nchunk;
  double* R;                 // [nchunk][p + 2]
  const int64_t* order;      // [nchunk] the chunks by their first row (null: as they lie): work unit u takes chunk order[u]
};
// fe2_gather_kernel: R[k, j] = sum_{q in unit k} v[row] src[id[row], j], j < nc, row = list[q] (list null:
// row = q), positions in ascending order; unit k is [start[k], start[k + 1]).
struct Fe2GatherArgs {
  const double* v;
  const int32_t* id;         // [n] the level of the other factor, validated on the host
  const double* src;         // row-major level matrix, leading dimension lds
  int64_t lds;
  int nc;
  const int64_t* list;
  const int64_t* start;      // [nunit + 1]
  int64_t nunit;
  double* R;                 // [nunit][nc]
  const int64_t* order;      // [nunit] or null, as Fe2ListSumArgs::order
};
// fe2_update_kernel: Y[l, j] = (S[l, j] - T[l, j]) / W_l, 0 where W_l = 0 or the level is pinned; the largest
// |change| and |Y| of column j go to stop[j] and stop[ldy + j] (integer max on the bit patterns).
struct Fe2UpdateArgs {
  const double* S;           // col-major sums S | t | W (p + 2 columns), leading dimension ldS
  const double* T;           // col-major (p + 1 columns), leading dimension ldS
  int64_t ldS, L;
  int p;
  const int32_t* pin;        // may be null
  double* Y;                 // row-major [L][ldy]
  int64_t ldy;
  unsigned long long* stop;  // [2 ldy]
};
// fe2_cross_kernel: per-slice partials of S_X' Y over the levels of both factors on fp64 MFMA;
// part [nslice[0] + nslice[1]][PR][PC] row-major, PR = 16 ceil(p / 16), PC = 16 ceil((p + 1) / 16).
struct Fe2CrossArgs {
  const double* S[2];
  int64_t ldS[2];
  const double* Y[2];
  int64_t L[2], slice_rows[2];
  int nslice[2];
  int p;
  int64_t ldy;
  double* part;
};
// fe2_offset_kernel: out_i = off_i + alpha[id1_i] + gamma[id2_i], zeros on the rows in [n, ld)
struct Fe2OffsetArgs {
  const double* off;         // may be null
  const double* alpha;
  const double* gamma;
  const int32_t* id1;
  const int32_t* id2;
  int64_t n, ld;
  double* out;
};
// fe2_effect_kernel: eff_l += Y[l, p] - sum_j Y[l, j] beta_j where W_l > 0.
// fe2_normalise_kernel: the shift of a level's component (gamma at the component's lowest factor-2 code)
// taken off gamma and added to alpha.
struct Fe2EffectArgs {
  const double* Y;
  int64_t ldy, L;
  int p;
  const double* W;           // [L]
  const double* beta;
  double* eff;               // [L]
};
struct Fe2NormArgs {
  double* alpha;
  double* gamma;
  const double* gamma_raw;   // a copy of gamma taken before the kernel
  const int32_t* comp1;      // [G] component of each level (-1: no rows)
  const int32_t* comp2;      // [H]
  const int32_t* low;        // [ncomp] lowest factor-2 code of each component
  int64_t G, H;
};
// fe2_meat_kernel: the rows S_g = Su_g - U_g a_g - Tu_g of the clustered meat into a design X [ld x p], y = 0
struct Fe2MeatArgs {
  const double* Su;          // col-major S | U | . of the u-weighted sums, leading dimension ld
  const double* Tu;          // col-major gather sums of u c, leading dimension ld
  const double* Y1;          // row-major [G][ldy]
  int64_t G, ld, ldy;
  int p;
  double* X;
  double* y;
};

// Arguments of the final-statistics pass (stats_kernel).
struct StatsArgs {
  const double* y;
  const double* m;
  const double* prior;
  const double* eta;    // MODE_IRLS: eta of the last pass; MODE_LM_RESID: X*coefs (or X != null below)
  const double* X;      // MODE_LM_RESID on a resident shard: eta = X*beta formed in the kernel
  int64_t ld;           //   (predict_kernel's order), so the residual pass reads X once and
  int p;                //   writes no eta
  const double* beta;
  int64_t n;
  int family, link, mode;
  double mu0, ybar;
  double* partials;     // [grid][NS]
  const double* ybar_dev;  // non-null: ybar read from the device (the LM device round trip, lm_chol_kernel)
  int beta_by_value;    // p <= STATS_BETA_MAX: beta travels in the kernel arguments (no H2D copy)
  double theta;         // FAM_NEGBIN: the dispersion parameter (before bv, which stays the last field)
  double bv[32];        //   beta_by_value: beta[0..p)
};
constexpr int STATS_BETA_MAX = 32;

// The negative binomial's theta terms (theta.hip theta_terms_kernel; sglm_nb_theta_terms' out[5] in this order).
enum ThetaTerm : int { T_SCORE = 0, T_INFO = 1, T_LL = 2, T_MOM = 3, T_SUMW = 4, THETA_NT = 5 };
struct ThetaArgs {
  const double* y;
  const double* eta;    // eta of the last pass (the buffer stats_kernel reads)
  const double* prior;  // may be null
  int64_t n;            // rows; rows >= n are never read
  int link;             // LNK_LOG, LNK_SQRT or LNK_IDENTITY
  double theta;
  double* partials;     // [grid][NS]: THETA_NT sums, zeros in the other slots (reduce_stats_kernel's layout)
};

// Multinomial logit (multinom.hip): K classes, class 0 the baseline, B [p x (K - 1)] col-major.
constexpr int MN_MAX_K = 16;
constexpr int MN_MAX_Q = 1024;  // (K - 1) p at most: the host solve's order, and B beside the rows' slots in LDS
// the scalars after the score in a workgroup's partial and in a pass's sums: sum pw log pi_y | sum pw | rows of
// positive weight whose y is no class code | the weighted class counts [MN_MAX_K]
enum MnScalar : int { MN_LL = 0, MN_SUMW = 1, MN_BAD = 2, MN_COUNT = 3, MN_NSC = 3 + MN_MAX_K };
enum MnMode : int { MN_DEV = 0, MN_FULL = 1 };  // the scalars alone | also P, and the score (or R for multinom_xtr_kernel)
struct MultinomArgs {
  const double* X;      // col-major, leading dimension ld; columns >= p are never read
  int64_t ld;
  int p;
  int K;
  int64_t n;            // rows; rows >= n are never read or stored
  const double* B;      // device [(K - 1) p]
  const double* y;      // class codes
  const double* prior;  // may be null
  double* P;            // MN_FULL: the probabilities [K][ld]
  double* R;            // MN_FULL past the fused shapes: R_ij = pw_i (1[y_i = j] - pi_ij), [K - 1][ld]
  double* part;         // [grid][stride]: the score [nscore] (MN_FULL), then the MN_NSC scalars
  int nscore;           // (K - 1) p, or 0 (MN_DEV)
  int stride;           // nscore + MN_NSC
};

}  // namespace sglm
