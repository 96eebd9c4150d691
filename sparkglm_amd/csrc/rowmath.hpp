// rowmath.hpp -- per-row family/link arithmetic of the IRLS pass (device side).
//
// Mirrors the reference's elementwise stage operation-for-operation:
//   link / lPrime / unlink  GLM.scala:190-251   (logit, probit, cloglog)
//   varianceBinomial        GLM.scala:125-129
//   w = 1/(V g'^2), z = eta + (y - mu) g' - offset      GLM.scala:289-290, 370-371
//   devBinomial row value   GLM.scala:166-167   (summed, times 2 on the host)
//   pearsonCalc             GLM.scala:90-101
//   llBinomial              GLM.scala:132-143   (Breeze Binomial(m.toInt, mu).logProbabilityOf)
// Extension families (gaussian, poisson, gamma with R's three links each; prior weights)
// follow R's family objects on the same skeleton.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "polygamma.hpp"

namespace sglm {

// Breeze Gaussian(0,1) as used by the probit link.
__device__ __forceinline__ double norm_cdf(double x) { return 0.5 * (1.0 + erf(x / sqrt(2.0))); }
__device__ __forceinline__ double norm_icdf(double q) { return 0.0 + 1.0 * sqrt(2.0) * erfinv(2.0 * q - 1.0); }
__device__ __forceinline__ double norm_pdf(double x) {
  double d = (x - 0.0) / 1.0;
  return exp(-d * d / 2.0 - (log(sqrt(2.0 * M_PI)) + log(1.0)));
}

// A polynomial coefficient materialised in an SGPR pair at its point of use (two s_mov_b32 on
// the scalar unit): without this the compiler hoists every coefficient of the fast paths out
// of the pass kernels' main loops into VGPRs, where they crowd out the Gram accumulators and
// spill to scratch -- and a scratch reload's vmcnt wait drains the LDS-DMA pipeline.
__device__ __forceinline__ double sc(double c) {
  asm volatile("" : "+s"(c));
  return c;
}

// Reciprocal of a positive normal x: v_rcp_f64 plus two Newton steps (quadratic convergence
// from the hardware estimate), ~1 ulp -- the fast paths below use it in place of the IEEE
// division sequence (div_scale / div_fmas / div_fixup), which they never need: their operands
// are bounded away from 0, denormals and infinity by the fast-path range checks.
__device__ __forceinline__ double rcp_pos(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}

// Natural log of a positive finite x (normal or denormal), ~2 ulp: x = m 2^k with
// m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m - 1)/(m + 1), |s| <= 0.1716, as
// 2s (1 + s^2/3 + ... + s^18/19) (truncation < 3e-17 relative).  The row fast paths use it
// for the deviance terms instead of libm's double-double log / log1p (about 3x fewer
// instructions); the per-row values differ from libm's by a few ulp, far inside the 1e-9
// parity tolerance on the summed deviance.
__device__ __forceinline__ double log_pos(double x) {
  double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
  int k = __builtin_amdgcn_frexp_exp(x);
  if (m < sc(0.70710678118654752440)) {
    m = m + m;
    k -= 1;
  }
  const double f = m - 1.0;
  const double s = f * rcp_pos(m + 1.0);
  const double z = s * s;
  // (Horner: Estrin's scheme, dependency depth 4 instead of 9, measured +-0 -- not kept)
  double q = sc(1.0 / 19.0);
  q = fma(q, z, sc(1.0 / 17.0));
  q = fma(q, z, sc(1.0 / 15.0));
  q = fma(q, z, sc(1.0 / 13.0));
  q = fma(q, z, sc(1.0 / 11.0));
  q = fma(q, z, sc(1.0 / 9.0));
  q = fma(q, z, sc(1.0 / 7.0));
  q = fma(q, z, sc(1.0 / 5.0));
  q = fma(q, z, sc(1.0 / 3.0));
  const double lm = fma(2.0 * s, z * q, 2.0 * s);
  const double kd = (double)k;
  return fma(kd, sc(6.93147180559945286227e-01), fma(kd, sc(2.31904681384629955842e-17), lm));
}

// exp(x) for |x| < 708 (the fast paths' range checks guarantee it), ~2 ulp: x = k ln2 + r,
// |r| <= ln2/2, Taylor series to r^13 (truncation < 5e-18 relative), scaled by 2^k.  No
// overflow / underflow / NaN handling -- libm's exp carries that on every call.
__device__ __forceinline__ double exp_small(double x) {
  const double kf = rint(x * sc(1.44269504088896338700));
  double r = fma(-kf, sc(6.93147180559945286227e-01), x);
  r = fma(-kf, sc(2.31904681384629955842e-17), r);
  double q = sc(1.0 / 6227020800.0);  // 1/13!
  q = fma(q, r, sc(1.0 / 479001600.0));
  q = fma(q, r, sc(1.0 / 39916800.0));
  q = fma(q, r, sc(1.0 / 3628800.0));
  q = fma(q, r, sc(1.0 / 362880.0));
  q = fma(q, r, sc(1.0 / 40320.0));
  q = fma(q, r, sc(1.0 / 5040.0));
  q = fma(q, r, sc(1.0 / 720.0));
  q = fma(q, r, sc(1.0 / 120.0));
  q = fma(q, r, sc(1.0 / 24.0));
  q = fma(q, r, sc(1.0 / 6.0));
  q = fma(q, r, 0.5);
  q = fma(q, r, 1.0);
  q = fma(q, r, 1.0);
  return __builtin_amdgcn_ldexp(q, (int)kf);
}

__device__ __forceinline__ double link_fn(int fam, int lnk, double mu, double m) {
  if (fam == FAM_BINOMIAL) {
    if (lnk == LNK_LOGIT) return log(mu / (m + (-1.0 * mu)));
    if (lnk == LNK_PROBIT) return norm_icdf(mu / m);
    return log(-1.0 * log(1.0 + (-1.0 * (mu / m))));
  }
  if (fam == FAM_GAUSSIAN) return mu;
  if (fam == FAM_POISSON) return log(mu);
  return 1.0 / mu;
}

__device__ __forceinline__ double unlink_fn(int fam, int lnk, double eta, double m) {
  if (fam == FAM_BINOMIAL) {
    if (lnk == LNK_LOGIT) return m / (1.0 + exp(-1.0 * eta));
    if (lnk == LNK_PROBIT) return m * norm_cdf(eta);
    return m * (1.0 + (-1.0 * exp(-exp(eta))));
  }
  if (fam == FAM_GAUSSIAN) return eta;
  if (fam == FAM_POISSON) return exp(eta);
  return 1.0 / eta;
}

__device__ __forceinline__ double lprime_fn(int fam, int lnk, double mu, double m) {
  if (fam == FAM_BINOMIAL) {
    if (lnk == LNK_LOGIT) return m / (mu * (m + (-1.0 * mu)));
    if (lnk == LNK_PROBIT) return 1.0 / (m * norm_pdf(norm_icdf(mu / m)));
    return 1.0 / ((mu + (-1.0 * m)) * log(1.0 + (-1.0 * (mu / m))));
  }
  if (fam == FAM_GAUSSIAN) return 1.0;
  if (fam == FAM_POISSON) return 1.0 / mu;
  return -1.0 / (mu * mu);
}

// The extension families' links by the link alone (R's make.link: identity, log, inverse, sqrt) -- the
// non-canonical pairs (common.hpp noncanonical_pair).  link_fn / unlink_fn / lprime_fn above select by
// family and serve the binomial links and the canonical pairs only.
__device__ __forceinline__ double link_fn_x(int lnk, double mu) {
  if (lnk == LNK_IDENTITY) return mu;
  if (lnk == LNK_LOG) return log(mu);
  if (lnk == LNK_INVERSE) return 1.0 / mu;
  return sqrt(mu);
}
__device__ __forceinline__ double unlink_fn_x(int lnk, double eta) {
  if (lnk == LNK_IDENTITY) return eta;
  if (lnk == LNK_LOG) return exp(eta);
  if (lnk == LNK_INVERSE) return 1.0 / eta;
  return eta * eta;
}
__device__ __forceinline__ double lprime_fn_x(int lnk, double mu) {
  if (lnk == LNK_IDENTITY) return 1.0;
  if (lnk == LNK_LOG) return 1.0 / mu;
  if (lnk == LNK_INVERSE) return -1.0 / (mu * mu);
  return 0.5 / sqrt(mu);
}
// whether an instantiation's rows take the _x functions (a compile-time constant at every call site)
constexpr bool link_by_link(int fam, int lnk) { return lnk == LNK_RT || noncanonical_pair(fam, lnk); }

// The link of an instantiation: its template argument, or (LNK_RT) the run-time link of its arguments.
template <int LNK>
__device__ __forceinline__ int link_of(int rt_link) {
  return LNK == LNK_RT ? rt_link : LNK;
}

// R's validmu / valideta for the non-canonical pairs (common.hpp noncanonical_pair): gaussian needs a
// finite eta (inverse: eta != 0); poisson and gamma a finite mu > 0 (sqrt: eta > 0).  A row outside
// cannot be fitted -- the reference has no step-halving -- and pass_row_ref marks it with a NaN unit
// deviance (pass_row_ref_x), which costs the pass no accumulator and makes the drivers stop with SGLM_EINVAL.
__device__ __forceinline__ bool link_row_valid(int fam, int lnk, double eta, double mu) {
  if (fam == FAM_GAUSSIAN) return isfinite(eta) && !(lnk == LNK_INVERSE && eta == 0.0);
  return isfinite(mu) && mu > 0.0 && !(lnk == LNK_SQRT && !(eta > 0.0));
}

__device__ __forceinline__ double variance_fn(int fam, double mu, double m) {
  if (fam == FAM_BINOMIAL) return mu * (1.0 + (-1.0 * (mu / m)));
  if (fam == FAM_GAUSSIAN) return 1.0;
  if (fam == FAM_POISSON) return mu;
  return mu * mu;
}

// Breeze Binomial(n, p).logProbabilityOf(k) with n = m.toInt, k = y.toInt, p = mu.
__device__ __forceinline__ double binom_logpmf(double mval, double mu, double yval, double& bad) {
  int n = (int)mval, k = (int)yval;
  if (n <= 0 || k < 0 || k > n || mu < 0.0) { bad += 1.0; return 0.0; }
  if (mu == 0.0) return k == 0 ? 0.0 : -INFINITY;
  if (mu == 1.0) return k == n ? 0.0 : -INFINITY;
  return lgamma(n + 1.0) - lgamma(k + 1.0) - lgamma(n - k + 1.0) + k * log(mu) + (n - k) * log1p(-mu);
}

// Compensated (Neumaier) accumulation for the last, widest levels of the scalar reductions: at
// 1e9 rows a plain sum of ~256-2048 partials of a ~1e9 deviance carries ~1e-6 of rounding --
// GLM.scala:281's absolute tol -- so the iteration count would follow the summation order.
__device__ __forceinline__ void neumaier_add(double& s, double& c, double x) {
  const double t = s + x;
  c += (fabs(s) >= fabs(x)) ? (s - t) + x : (x - t) + s;
  s = t;
}

struct RowAcc {
  double s[NS];
};

// Poisson counts y < POIS_TAB that are integers take their per-row functions of y from tables
// built once per workgroup in LDS with the reference's own expressions (poisson_init_table,
// poisson_ylogy_table below).
constexpr int POIS_TAB = 256;

// Unit deviance row value: devBinomial (GLM.scala:166-167) and the R families; the
// family factor (2 for binomial / poisson / gamma) is applied on the host after summing.
__device__ __forceinline__ double unit_dev(int fam, double y, double mu, double m, double pw) {
  if (fam == FAM_BINOMIAL) {
    double my = m + (-1.0 * y);
    return pw * ((y * log(fmax(y, 1.0) / mu)) + (my * log(fmax(my, 1.0) / (m + (-1.0 * mu)))));
  }
  if (fam == FAM_GAUSSIAN) {
    double e = y - mu;
    return pw * (e * e);
  }
  if (fam == FAM_POISSON) return pw * ((y > 0.0 ? y * log(y / mu) : 0.0) - (y - mu));
  return pw * (-(log(y / mu) - (y - mu) / mu));
}

// ---- negative binomial with a fixed theta (MASS::negative.binomial(theta)) ----
// V = mu + mu^2 / theta; unit deviance y log(max(y, 1) / mu) - (y + theta) log((y + theta) / (mu + theta)) (family
// factor 2); the log-density of R's dnbinom(y, theta, mu = mu).
__device__ __forceinline__ double nb_variance(double mu, double theta) { return mu + (mu * mu) / theta; }
__device__ __forceinline__ double nb_unit_dev(double y, double mu, double pw, double theta) {
  return pw * ((y * log(fmax(y, 1.0) / mu)) - ((y + theta) * log((y + theta) / (mu + theta))));
}
__device__ __forceinline__ double nb_loglik_row(double y, double mu, double theta) {
  return ((((lgamma(theta + y) - lgamma(theta)) - lgamma(y + 1.0)) + theta * log(theta)) +
          y * log(mu + (y == 0.0 ? 1.0 : 0.0))) - (theta + y) * log(theta + mu);
}

// The reference operation order (zwCreateBinomial GLM.scala:359-395) of every row the fast paths below do
// not take -- init modes, m != 1, probit / cloglog, the non-canonical pairs, the negative binomial, rows
// outside the fast paths' ranges.  row_core is its one spelling in the pass: mu from eta (IRLS) or from mu0
// (the init modes: eta = link(mu0), the offset ignored, GLM.scala:264-270), g', V and the working weight.
// by_link (link_by_link: the links selected by link) and nb (the negative binomial variance at theta) are
// compile-time constants (CT<>) in the pass's rows, whose instantiations then hold one set of links each, and
// run-time bools in the diagnostics and fixed-effects rows (influence_row, fe.hip fe_row), which serve every
// (family, link) from one function.
template <bool V>
struct CT {
  constexpr operator bool() const { return V; }
};
struct RowCore {
  double eta, mu, g, v, w;
};
template <class BYLINK, class NB>
__device__ __forceinline__ RowCore row_core(BYLINK by_link, NB nb, int fam, int lnk, int mode, double eta, double m,
                                            double pw, double mu0, double theta) {
  double mu;
  if (mode == MODE_IRLS) {
    mu = by_link ? unlink_fn_x(lnk, eta) : unlink_fn(fam, lnk, eta, m);
  } else {
    eta = by_link ? link_fn_x(lnk, mu0) : link_fn(fam, lnk, mu0, m);
    mu = (mode == MODE_INIT_SINGLE) ? mu0 : (by_link ? unlink_fn_x(lnk, eta) : unlink_fn(fam, lnk, eta, m));
  }
  const double g = by_link ? lprime_fn_x(lnk, mu) : lprime_fn(fam, lnk, mu, m);
  const double v = nb ? nb_variance(mu, theta) : variance_fn(fam, mu, m);
  return RowCore{eta, mu, g, v, pw * (1.0 / (v * (g * g)))};
}
// w z, z = eta + (y - mu) g' - offset (GLM.scala:289-290, 370-371)
__device__ __forceinline__ double working_wz(double w, double eta, double y, double mu, double g, double off) {
  const double z = (eta + ((y + (-1.0 * mu)) * g)) + (-1.0 * off);
  return w * z;
}

// The pass's reference rows: the core plus the unit deviance (devBinomial :162-170).  Out of line: their libm
// calls' constants would otherwise be hoisted into the pass kernels' main loops and take registers from the
// Gram accumulators.
struct RowWZ {
  double w, wz, dev;
};
__device__ __forceinline__ RowWZ row_wz(const RowCore& c, double y, double off) {
  return RowWZ{c.w, working_wz(c.w, c.eta, y, c.mu, c.g, off), 0.0};
}
// fitMultipleBinomial re-derives mu = unlink(link(ybar)) only inside zwCreateBinomial; its null deviance is
// taken at mu0 = ybar itself (GLM.scala:424-444)
__device__ __noinline__ RowWZ pass_row_ref(int fam, int lnk, int mode, double eta, double y, double m, double off,
                                           double pw, double mu0) {
  const RowCore c = row_core(CT<false>{}, CT<false>{}, fam, lnk, mode, eta, m, pw, mu0, 0.0);
  RowWZ r = row_wz(c, y, off);
  r.dev = unit_dev(fam, y, mode == MODE_IRLS ? c.mu : mu0, m, pw);
  return r;
}
// The non-canonical pairs: the validity of the row (link_row_valid) is carried as a NaN unit deviance.  An
// invalid row yields NaN / Inf arithmetic only -- no index depends on mu.
__device__ __noinline__ RowWZ pass_row_ref_x(int fam, int lnk, int mode, double eta, double y, double m, double off,
                                             double pw, double mu0) {
  const RowCore c = row_core(CT<true>{}, CT<false>{}, fam, lnk, mode, eta, m, pw, mu0, 0.0);
  RowWZ r = row_wz(c, y, off);
  r.dev = link_row_valid(fam, lnk, c.eta, c.mu) ? unit_dev(fam, y, mode == MODE_IRLS ? c.mu : mu0, m, pw) : NAN;
  return r;
}
// The negative binomial: its variance and deviance; the row's validity is the poisson rows' rule
// (link_row_valid: mu finite and > 0, sqrt needs eta > 0).
__device__ __noinline__ RowWZ pass_row_ref_nb(int lnk, int mode, double eta, double y, double off, double pw,
                                              double mu0, double theta) {
  const RowCore c = row_core(CT<true>{}, CT<true>{}, FAM_NEGBIN, lnk, mode, eta, 1.0, pw, mu0, theta);
  RowWZ r = row_wz(c, y, off);
  r.dev = link_row_valid(FAM_NEGBIN, lnk, c.eta, c.mu) ? nb_unit_dev(y, mode == MODE_IRLS ? c.mu : mu0, pw, theta) : NAN;
  return r;
}

// The initial pass of a binomial fit without m (GLM.scala:263-272, 429-444): mu = mu0
// (fitSingle) or unlink(link(mu0)) (fitMultiple) is the same for every row, so link, lPrime and
// the variance are invariants of the pass; per row only z and the deviance remain.
// max(y, 1) = max(1 - y, 1) = 1 for 0 <= y <= 1, so devBinomial's logs are invariant too -- the
// expressions are the reference's own, operation for operation (pass_row_ref), so the rows come
// out bitwise pass_row_ref's.  v = {e0, mu, g, w0, l1, l0}.
struct InitConst {
  double v[6];
};
// (by_link: the non-canonical pairs' links, link_by_link -- a compile-time constant at the call sites)
__device__ __forceinline__ InitConst init_const(int fam, int lnk, int mode, double mu0, bool by_link = false) {
  InitConst c;
  const double e0 = by_link ? link_fn_x(lnk, mu0) : link_fn(fam, lnk, mu0, 1.0);
  const double mu = (mode == MODE_INIT_SINGLE) ? mu0 : (by_link ? unlink_fn_x(lnk, e0) : unlink_fn(fam, lnk, e0, 1.0));
  const double g = by_link ? lprime_fn_x(lnk, mu) : lprime_fn(fam, lnk, mu, 1.0);
  c.v[0] = e0;
  c.v[1] = mu;
  c.v[2] = g;
  c.v[3] = 1.0 / (variance_fn(fam, mu, 1.0) * (g * g));
  c.v[4] = fam == FAM_BINOMIAL ? log(1.0 / mu0) : 0.0;
  c.v[5] = fam == FAM_BINOMIAL ? log(1.0 / (1.0 + (-1.0 * mu0))) : 0.0;
  return c;
}
// the fused kernels' initial passes take these constants from LDS (computed once per workgroup)
__device__ __forceinline__ bool init_fast_row(int fam, int mode, bool has_m) {
  return fam == FAM_BINOMIAL && (mode == MODE_INIT_SINGLE || mode == MODE_INIT_MULTI) && !has_m;
}
__device__ __forceinline__ void pass_row_init(const double* c, double y, double off, double pw, double& w, double& wz,
                                              double& s_dev, double& s_aux) {
  w = pw * c[3];
  const double z = (c[0] + ((y + (-1.0 * c[1])) * c[2])) + (-1.0 * off);
  wz = w * z;
  const double my = 1.0 + (-1.0 * y);
  s_dev += pw * ((y * c[4]) + (my * c[5]));
  s_aux += pw;
}

// ---- the inline fast paths: one function per (family, link), shared by the pass (pass_row), the pass
// with in-pass final statistics (pass_row_stats, STATS) and stats_kernel (stats_row) ----
// Each sums w, w z, the unit deviance and sum pw; with STATS also pearsonCalc and the family's loglik
// ingredients at the same mu, from the same exp / reciprocal / log.  Its SGLM_*_FAST condition is the range
// its forms hold in; other rows take the reference order.  (Macros: the conditions then join the callers'
// short-circuit chains as if spelled there -- as functions they compiled to other branch structures in
// the pass kernels.)

// Logit, m = 1: the reference's expressions (GLM.scala:190-204, 125-129, 162-170, 289-290)
// in an algebraically identical form with one exp, one division and one log1p:
//   t = 1/(1+e), e = exp(-eta):  mu = t,  V = e t^2,  g' = 1/V,  w = V,  w*z = V (eta - off) + (y - mu)
//   dev row = y log(1/mu) + (1-y) log(1/(1-mu)) = log1p(e) + (1-y) eta
// Inside |eta| < 8 both forms agree to ~1e-13 relative per row (1 - mu >= 3e-4, no
// cancellation); outside it, and for m != 1, the reference operation order applies.
// u = 1 + e lies in (1, 2982): t = 1/u by rcp_pos, and log1p(e) = log(u) + (e - (u - 1))/u
// (the rounding of u corrected to first order, as libm's log1p does).
// STATS: Breeze's Binomial(1, mu).logProbabilityOf(k) = k log mu + (1-k) log(1-mu) with log mu = -log1p(e),
// log(1-mu) = -eta - log1p(e); |eta| < 8 keeps mu off 0 and 1 (no special cases, k in {0, 1}).
#define SGLM_LOGIT_FAST(eta, y) (fabs(eta) < 8.0 && (y) >= 0.0 && (y) <= 1.0)
// The row in two halves, so that a caller can hand w and w*z on before the deviance's log is formed
// (K1r's row stage, fused.hpp row_stage_r): logit_row_wz leaves e, u, t and v for logit_row_dev.
struct LogitEUT {
  double e, u, t, v;
};
__device__ __forceinline__ bool logit_fast_row(int mode, bool has_m, double eta, double y) {
  return mode == MODE_IRLS && !has_m && SGLM_LOGIT_FAST(eta, y);  // pass_row's condition
}
__device__ __forceinline__ LogitEUT logit_row_wz(double eta, double y, double off, double pw, bool small_exp,
                                                 double& w, double& wz) {
  LogitEUT c;
  c.e = small_exp ? exp_small(-eta) : exp(-eta);
  c.u = 1.0 + c.e;
  c.t = rcp_pos(c.u);
  c.v = c.e * c.t * c.t;
  w = pw * c.v;
  wz = pw * (c.v * (eta - off) + (y - c.t));
  return c;
}
// (returns L = log1p(e) = -log(mu))
__device__ __forceinline__ double logit_row_dev(const LogitEUT& c, double eta, double y, double pw, double& s_dev,
                                                double& s_aux) {
  const double L = fma(c.e - (c.u - 1.0), c.t, log_pos(c.u));
  s_dev += pw * (L + (1.0 - y) * eta);
  s_aux += pw;
  return L;
}
template <bool STATS>
__device__ __forceinline__ void logit_row(double eta, double y, double off, double pw, bool small_exp, double& w,
                                          double& wz, double& s_dev, double& s_aux, double& s_pear, double& s_ll) {
  const LogitEUT c = logit_row_wz(eta, y, off, pw, small_exp, w, wz);
  const double L = logit_row_dev(c, eta, y, pw, s_dev, s_aux);
  if constexpr (STATS) {
    const double r = y - c.t;
    s_pear += pw * (r * r) * rcp_pos(c.v);
    s_ll += pw * ((int)y == 1 ? -L : -L - eta);
  }
}

// y log y - y eta of a count row (Poisson, negative binomial): y log y from the narrow kernel's LDS table of
// k log k for the integer counts k < POIS_TAB (poisson_ylogy_table), so that those rows need no log; other
// rows (no table, non-integer or large y) take log_pos.
__device__ __forceinline__ double ylogy_minus_yeta(const double* ylogy, double y, double eta) {
  if (ylogy && y < (double)POIS_TAB && y == floor(y)) return ylogy[(int)y] - y * eta;
  return y > 0.0 ? y * (log_pos(y) - eta) : 0.0;
}

// Poisson / log (R's poisson()): mu = exp(eta), g' = 1/mu, V = mu, so
//   w = 1/(V g'^2) = mu,  w*z = mu (eta - off) + (y - mu),
//   dev row = y log(y/mu) - (y - mu) = (y log y - y eta) - (y - mu)
// -- one exp and one log (or a table look-up), no divisions; the reference operation order
// agrees to a few ulp per row, and it still runs where exp could overflow.  The deviance stays
// a per-row sum of terms of the size of the row's own deviance -- what GLM.scala:452's absolute tol
// on the change needs (a round-3 form summed -y eta - (y - mu) per row and added sum y log y once
// per pass: with counts ~1e3 over 1e8 rows its terms reached ~1e12 in total and their rounding,
// ~1e-4, swamped tol 1e-6).
// STATS: pearsonCalc (R's variance V = mu) and the mu-dependent part of R's dpois
// log-density, y log mu - mu with log mu = eta.  The per-row constant -lgamma(y + 1) does not depend on the
// fit: the initial pass sums pw lgamma(y + 1) once into S_AUX2 (init_stats_const) and the engine subtracts it.
#define SGLM_POISSON_LOG_FAST(eta, y) (fabs(eta) < 700.0 && (y) >= 0.0 && (y) < 1e300)
template <bool STATS>
__device__ __forceinline__ void poisson_log_row(double eta, double y, double off, double pw, bool small_exp,
                                                const double* ylogy, double& w, double& wz, double& s_dev,
                                                double& s_aux, double& s_pear, double& s_ll) {
  const double mu = small_exp ? exp_small(eta) : exp(eta);
  w = pw * mu;
  wz = pw * (mu * (eta - off) + (y - mu));
  s_dev += pw * (ylogy_minus_yeta(ylogy, y, eta) - (y - mu));
  s_aux += pw;
  if constexpr (STATS) {
    const double r = y - mu;
    s_pear += pw * (r * r) * rcp_pos(mu);
    s_ll += pw * (y * eta - mu);
  }
}

// Gamma / inverse (R's Gamma()): mu = 1/eta, g' = -1/mu^2, V = mu^2, so
//   w = mu^2,  w*z = mu^2 (eta - off) - (y - mu),
//   dev row = -(log(y/mu) - (y - mu)/mu) = -(log(y eta) - (y eta - 1))
// -- one reciprocal and one log instead of four divisions and a log (the range checks keep
// eta, y and y eta normal and finite for rcp_pos / log_pos).
// STATS: pearsonCalc (V = mu^2: (y - mu)^2 / mu^2 = (y - mu)^2 eta^2) and R's Gamma loglik ingredients
// sum pw y / mu = sum pw y eta (s_aux0) and sum pw log mu = sum pw log y - sum pw log(y eta) (the pass sums
// the second term, s_lye, which its deviance already evaluates; the fit-constant sum pw log y -- also S_LL
// itself -- comes from the initial pass, init_stats_const).
#define SGLM_GAMMA_INVERSE_FAST(eta, y) ((eta) > 1e-150 && (eta) < 1e150 && (y) > 1e-150 && (y) < 1e150)
template <bool STATS>
__device__ __forceinline__ void gamma_inverse_row(double eta, double y, double off, double pw, double& w, double& wz,
                                                  double& s_dev, double& s_aux, double& s_pear, double& s_aux0,
                                                  double& s_lye) {
  const double mu = rcp_pos(eta);
  const double mu2 = mu * mu;
  const double ye = y * eta;
  w = pw * mu2;
  wz = pw * (mu2 * (eta - off) - (y - mu));
  const double L = log_pos(ye);
  s_dev += pw * (-(L - (ye - 1.0)));
  s_aux += pw;
  if constexpr (STATS) {
    const double r = y - mu;
    s_pear += pw * (r * r) * (eta * eta);
    s_aux0 += pw * ye;
    s_lye += pw * L;
  }
}

// The row stage of the fused pass (zwCreateBinomial, GLM.scala:359-395 / the single-
// partition loop body GLM.scala:282-301): w and w*z for the Gramian, and the deviance.
// LM gram mode: w = 1, z = y, and the sums of y and of rows (LM.scala:142-155, 167).
// small_exp and init_fast are compile-time constants at every call site.
// small_exp selects exp_small over libm's exp.  Every narrow variant (p <= 64) passes true: round 4
// measured it -1 % at p <= 32 and +4 % at p = 64 on that round's narrow kernel; round 5's rework of
// the narrow pass (row stage at raised issue priority, block pairs at p > 32) set it for every width
// without a separate p = 64 A/B of this choice.  K1r's row stage passes true at every width (fused.hpp
// row_stage_r) and K1 at 16 column blocks (P16 == 16, p = 241..256): exp_small runs on the 256-column
// paths.  K1 below 16 column blocks and the wide row kernel leave it off (libm's exp).
// tests/test_gpu_rowmath.py holds every instantiation's rows to the bars derived from these primitives.
// ylogy: the narrow kernel's IRLS passes' table of the counts' y log y (ylogy_minus_yeta).
__device__ __forceinline__ void pass_row(int fam, int lnk, int mode, double eta, double y, double m, double off,
                                         double pw, double mu0, double ybar, bool has_m, double& w, double& wz,
                                         double& s_dev, double& s_aux, bool small_exp = false,
                                         bool init_fast = false, const double* ylogy = nullptr, int rt_link = 0,
                                         double theta = 0.0, bool logit_fast_elsewhere = false) {
  (void)ybar;
  double nil;  // the statistics sums of the fast paths: not formed here (STATS = false)
  // (logit_fast_elsewhere: the caller took the logit fast rows itself, in halves -- K1r's row stage)
  if (!logit_fast_elsewhere && fam == FAM_BINOMIAL && lnk == LNK_LOGIT && mode == MODE_IRLS && !has_m &&
      SGLM_LOGIT_FAST(eta, y)) {
    logit_row<false>(eta, y, off, pw, small_exp, w, wz, s_dev, s_aux, nil, nil);
    return;
  }
  if (fam == FAM_POISSON && lnk == LNK_LOG && mode == MODE_IRLS && SGLM_POISSON_LOG_FAST(eta, y)) {
    poisson_log_row<false>(eta, y, off, pw, small_exp, ylogy, w, wz, s_dev, s_aux, nil, nil);
    return;
  }
  if (fam == FAM_GAMMA && lnk == LNK_INVERSE && mode == MODE_IRLS && SGLM_GAMMA_INVERSE_FAST(eta, y)) {
    gamma_inverse_row<false>(eta, y, off, pw, w, wz, s_dev, s_aux, nil, nil, nil);
    return;
  }
  if (fam == FAM_GAMMA && lnk == LNK_LOG && mode == MODE_IRLS && fabs(eta) < 300.0 && y > 1e-150 && y < 1e150) {
    // Gamma / log (R's Gamma(link = "log")): mu = exp(eta), g' = 1/mu, V = mu^2, so the working weight
    // is the prior weight itself, and with r = exp(-eta) = 1/mu
    //   w = pw,  w*z = pw ((eta - off) + (y r - 1)),
    //   dev row = -(log(y/mu) - (y - mu)/mu) = -(log(y r) - (y r - 1))
    // -- one exp and one log, no division.  |eta| < 300 keeps r and y r normal and finite for log_pos
    // and implies the row's validity (mu = exp(eta) finite and > 0); other rows take pass_row_ref.
    const double r = small_exp ? exp_small(-eta) : exp(-eta);
    const double yr = y * r;
    w = pw;
    wz = pw * ((eta - off) + (yr - 1.0));
    s_dev += pw * (-(log_pos(yr) - (yr - 1.0)));
    s_aux += pw;
    return;
  }
  if (fam == FAM_NEGBIN && lnk == LNK_LOG && mode == MODE_IRLS && fabs(eta) < 300.0 && y >= 0.0 && y < 1e150 &&
      theta > 1e-150 && theta < 1e150) {
    // Negative binomial / log (MASS::negative.binomial(theta)): mu = exp(eta), g' = 1/mu, V = mu + mu^2/theta, so
    // with r = 1/(mu + theta) and t = theta r
    //   w = 1/(V g'^2) = mu theta/(mu + theta) = mu t,  w*z = mu t (eta - off) + (y - mu) t,
    //   dev row = y log(max(y, 1)/mu) - (y + theta) log((y + theta)/(mu + theta))
    //           = (y log y - y eta) - (y + theta) log((y + theta) r)
    // -- one exp, one reciprocal and one log (y log y from the narrow kernel's table of counts, or a second
    // log).  The range checks keep mu + theta in (1e-150, 2e150), t in (5e-281, 1] and (y + theta) r in
    // (5e-301, 2e300): normal operands for rcp_pos / log_pos; they imply the row's validity (mu finite, > 0).
    // Other rows take pass_row_ref_nb.
    const double mu = small_exp ? exp_small(eta) : exp(eta);
    const double r = rcp_pos(mu + theta);
    const double t = theta * r;
    const double wt = mu * t;
    w = pw * wt;
    wz = pw * (wt * (eta - off) + (y - mu) * t);
    const double d0 = ylogy_minus_yeta(ylogy, y, eta);
    const double yt = y + theta;
    s_dev += pw * (d0 - yt * log_pos(yt * r));
    s_aux += pw;
    return;
  }
  if (mode == MODE_LM_GRAM) {
    w = 1.0;
    wz = y;
    s_dev += y;
    s_aux += 1.0;
    return;
  }
  if (init_fast && fam == FAM_BINOMIAL && mode != MODE_IRLS && mode != MODE_LM_GRAM && !has_m && y >= 0.0 &&
      y <= 1.0) {
    // (init_fast: set by the narrow kernel's non-IRLS instantiation only, whose loop the
    // invariants are hoisted out of; the fused kernels take them from LDS, pass_row_init.)
    const InitConst c = init_const(fam, lnk, mode, mu0);
    pass_row_init(c.v, y, off, pw, w, wz, s_dev, s_aux);
    return;
  }
  // (LNK_RT instantiations: every row takes the reference functions at the arguments' link)
  const RowWZ r = fam == FAM_NEGBIN ? pass_row_ref_nb(lnk == LNK_RT ? rt_link : lnk, mode, eta, y, off, pw, mu0, theta)
                  : link_by_link(fam, lnk) ? pass_row_ref_x(fam, lnk == LNK_RT ? rt_link : lnk, mode, eta, y, m, off, pw, mu0)
                                         : pass_row_ref(fam, lnk, mode, eta, y, m, off, pw, mu0);
  w = r.w;
  wz = r.wz;
  s_dev += r.dev;
  s_aux += pw;
}

// The reference operation order of the final statistics (pearsonCalc GLM.scala:90-101, devBinomial
// :162-170), out of line like pass_row_ref: rows the inline fast path of stats_row does not take.
// stats_core is its one spelling -- mu (returned), V, the unit deviance, Pearson and sum pw into a zeroed
// acc -- with row_core's BYLINK / NB; the family log-likelihood terms follow in each function.
// init modes (a fit that stops before its first solve): the statistics at mu0 itself, as
// pearsonCalc / llBinomial see the broadcast ybar (GLM.scala:424-426, 465-466)
template <bool BYLINK, bool NB>
__device__ __forceinline__ double stats_core(RowAcc& acc, int fam, int lnk, int mode, double eta, double y, double m,
                                             double pw, double mu0, double theta) {
#pragma unroll
  for (int k = 0; k < NS; ++k) acc.s[k] = 0.0;
  const double mu = (mode == MODE_IRLS) ? (BYLINK ? unlink_fn_x(lnk, eta) : unlink_fn(fam, lnk, eta, m)) : mu0;
  const double v = NB ? nb_variance(mu, theta) : variance_fn(fam, mu, m);
  const double r = y + (-1.0 * mu);
  acc.s[S_DEV] += NB ? nb_unit_dev(y, mu, pw, theta) : unit_dev(fam, y, mu, m, pw);
  acc.s[S_PEARSON] += pw * (r * r) / v;
  acc.s[S_SUMW] += pw;
  return mu;
}
// the R families' loglik ingredients (gaussian, poisson, gamma)
__device__ __forceinline__ void ext_loglik_terms(RowAcc& acc, int fam, double y, double mu, double pw) {
  if (fam == FAM_GAUSSIAN) {
    acc.s[S_LL] += log(pw);
  } else if (fam == FAM_POISSON) {
    acc.s[S_LL] += pw * (y * log(mu) - mu - lgamma(y + 1.0));
  } else {
    acc.s[S_LL] += pw * log(y);
    acc.s[S_AUX0] += pw * (y / mu);
    acc.s[S_AUX1] += pw * log(mu);
  }
}
// the binomial links and the canonical pairs: llBinomial (GLM.scala:132-143)
__device__ __noinline__ RowAcc stats_row_ref(int fam, int lnk, int mode, double eta, double y, double m, double pw,
                                             double mu0, bool has_m) {
  RowAcc acc;
  const double mu = stats_core<false, false>(acc, fam, lnk, mode, eta, y, m, pw, mu0, 0.0);
  if (fam == FAM_BINOMIAL) {
    double bad = 0.0, ll;
    if (has_m) {
      ll = binom_logpmf(m, mu, y, bad);
    } else {  // m == 1: the lgamma terms vanish; same special cases as Breeze
      const int k = (int)y;
      if (k < 0 || k > 1 || mu < 0.0) { bad = 1.0; ll = 0.0; }
      else if (mu == 0.0) ll = k == 0 ? 0.0 : -INFINITY;
      else if (mu == 1.0) ll = k == 1 ? 0.0 : -INFINITY;
      else ll = k * log(mu) + (1 - k) * log1p(-mu);
    }
    acc.s[S_LL] += pw * ll;
    acc.s[S_BAD] += bad;
  } else {
    ext_loglik_terms(acc, fam, y, mu, pw);
  }
  return acc;
}
// the non-canonical pairs (extension families only): mu by the link
__device__ __noinline__ RowAcc stats_row_ref_x(int fam, int lnk, int mode, double eta, double y, double pw,
                                               double mu0) {
  RowAcc acc;
  const double mu = stats_core<true, false>(acc, fam, lnk, mode, eta, y, 1.0, pw, mu0, 0.0);
  ext_loglik_terms(acc, fam, y, mu, pw);
  return acc;
}
// the negative binomial: S_LL is the whole log-likelihood sum pw dnbinom(y, theta, mu, log)
__device__ __noinline__ RowAcc stats_row_ref_nb(int lnk, int mode, double eta, double y, double pw, double mu0,
                                                double theta) {
  RowAcc acc;
  const double mu = stats_core<true, true>(acc, FAM_NEGBIN, lnk, mode, eta, y, 1.0, pw, mu0, theta);
  acc.s[S_LL] += pw * nb_loglik_row(y, mu, theta);
  return acc;
}

// Final statistics of one row at the converged mu: pearsonCalc (GLM.scala:90-101),
// llBinomial (GLM.scala:132-143) and the extension families' loglik ingredients; LM
// mode: SSE / SSR / SST terms of rowPartitionedSSE (LM.scala:172-175) with eta = X*coefs.
__device__ __forceinline__ void stats_row(int fam, int lnk, int mode, double eta, double y, double m, double pw,
                                          double mu0, double ybar, bool has_m, RowAcc& acc) {
  if (mode == MODE_LM_RESID) {
    const double e = y - eta, t = eta + (-1.0 * ybar), b = y + (-1.0 * ybar);
    acc.s[S_DEV] += e * e;
    acc.s[S_PEARSON] += t * t;
    acc.s[S_LL] += b * b;
    acc.s[S_SUMW] += 1.0;
    return;
  }
  if (fam == FAM_BINOMIAL && lnk == LNK_LOGIT && mode == MODE_IRLS && !has_m && SGLM_LOGIT_FAST(eta, y)) {
    double w, wz;  // not used here
    logit_row<true>(eta, y, 0.0, pw, true, w, wz, acc.s[S_DEV], acc.s[S_SUMW], acc.s[S_PEARSON], acc.s[S_LL]);
    return;
  }
  const RowAcc r = stats_row_ref(fam, lnk, mode, eta, y, m, pw, mu0, has_m);
#pragma unroll
  for (int k = 0; k < NS; ++k) acc.s[k] += r.s[k];
}

// Rows outside the in-pass statistics' fast ranges: both reference-order functions and the
// family's statistics slots (s2, s3, s4: StatsSlots), in ONE out-of-line call -- two calls (or
// an inlined lgamma) around the kernel's live Gram accumulators made the compiler spill them.
struct RowStats {
  double w, wz, dev, s2, s3, s4;
};
__device__ __noinline__ RowStats stats_row_fallback(int fam, int lnk, double eta, double y, double off, double pw) {
  const RowWZ r = pass_row_ref(fam, lnk, MODE_IRLS, eta, y, 1.0, off, pw, 0.0);
  const RowAcc a = stats_row_ref(fam, lnk, MODE_IRLS, eta, y, 1.0, pw, 0.0, false);
  RowStats o;
  o.w = r.w;
  o.wz = r.wz;
  o.dev = r.dev;
  o.s2 = a.s[S_PEARSON];
  if (fam == FAM_BINOMIAL) {
    o.s3 = a.s[S_LL];
    o.s4 = a.s[S_BAD];
  } else if (fam == FAM_POISSON) {
    o.s3 = a.s[S_LL] + pw * lgamma(y + 1.0);  // the constant part is subtracted once per fit
    o.s4 = 0.0;
  } else {
    o.s3 = a.s[S_AUX0];
    o.s4 = a.s[S_LL] - a.s[S_AUX1];  // pw log y - pw log mu = pw log(y / mu)
  }
  return o;
}

// In-pass final statistics (PassArgs::stats_in_pass; common.hpp stats_in_pass_family): the IRLS row stage
// of pass_row plus the final statistics' terms at the same mu -- the pass then needs no eta store and no
// stats_kernel pass.  Three family-specific accumulators (s2, s3, s4) that the kernel stores into the slots
// StatsSlots names: logit (Pearson, loglik, bad), Poisson (Pearson, loglik part, -), Gamma (Pearson, AUX0,
// sum pw log(y eta) -> AUX1 on the host).  Rows outside the fast range take stats_row_fallback.
template <int FAM>
struct StatsSlots {
  static constexpr int S2 = S_PEARSON;
  static constexpr int S3 = FAM == FAM_GAMMA ? S_AUX0 : S_LL;
  static constexpr int S4 = FAM == FAM_GAMMA ? S_AUX1 : (FAM == FAM_BINOMIAL ? S_BAD : -1);
};
template <int FAM>
__device__ __forceinline__ void pass_row_stats(double eta, double y, double off, double pw, double& w, double& wz,
                                               double& s_dev, double& s_aux, double& s2, double& s3, double& s4,
                                               bool small_exp, const double* ylogy = nullptr) {
  static_assert(FAM == FAM_BINOMIAL || FAM == FAM_POISSON || FAM == FAM_GAMMA, "stats_in_pass_family");
  constexpr int LNK = FAM == FAM_BINOMIAL ? LNK_LOGIT : (FAM == FAM_POISSON ? LNK_LOG : LNK_INVERSE);
  if constexpr (FAM == FAM_BINOMIAL) {
    if (SGLM_LOGIT_FAST(eta, y)) return logit_row<true>(eta, y, off, pw, small_exp, w, wz, s_dev, s_aux, s2, s3);
  } else if constexpr (FAM == FAM_POISSON) {
    if (SGLM_POISSON_LOG_FAST(eta, y))
      return poisson_log_row<true>(eta, y, off, pw, small_exp, ylogy, w, wz, s_dev, s_aux, s2, s3);
  } else {
    if (SGLM_GAMMA_INVERSE_FAST(eta, y)) return gamma_inverse_row<true>(eta, y, off, pw, w, wz, s_dev, s_aux, s2, s3, s4);
  }
  const RowStats r = stats_row_fallback(FAM, LNK, eta, y, off, pw);
  w = r.w;
  wz = r.wz;
  s_dev += r.dev;
  s_aux += pw;
  s2 += r.s2;
  s3 += r.s3;
  if constexpr (StatsSlots<FAM>::S4 >= 0) s4 += r.s4;
}

// The per-fit constants of the in-pass statistics, summed by the initial pass into S_AUX2:
// Poisson sum pw lgamma(y + 1) (R's dpois), Gamma sum pw log y (R's dgamma).
__device__ __noinline__ double init_stats_const_ref(int fam, double y, double pw) {
  return fam == FAM_POISSON ? pw * lgamma(y + 1.0) : pw * log(y);
}
template <int FAM>
__device__ __forceinline__ double init_stats_const(double y, double pw) {
  if constexpr (FAM == FAM_POISSON || FAM == FAM_GAMMA) return init_stats_const_ref(FAM, y, pw);
  return 0.0;
}

// The initial pass of a Poisson fit (mu = mu0 for every row, GLM.scala:263-272, 429-444, R's
// poisson()): per row, pass_row_ref needs log(y / mu0) for the unit deviance, and the in-pass
// statistics' constant needs lgamma(y + 1) (init_stats_const) -- two libm calls on the 16 of 64
// lanes of a p = 64 narrow pass.  Counts y are small integers, so the two functions of k = y are
// tabulated once per workgroup for k < POIS_TAB with the very same expressions
// (tab[k] = (k > 0 ? k log(k / mu0) : 0) - (k - mu0), tab[T + k] = lgamma(k + 1)); a row then
// multiplies by its prior weight exactly where the reference expressions do, so the rows are
// bitwise pass_row_ref's.  Other rows (non-integer or large y) take the reference path.
__device__ __forceinline__ void poisson_init_table(double* tab, double mu0, int k) {
  const double y = (double)k;
  tab[k] = (y > 0.0 ? y * log(y / mu0) : 0.0) - (y - mu0);
  tab[POIS_TAB + k] = lgamma(y + 1.0);
}
// The IRLS passes' table (ylogy_minus_yeta): k log k, 0 at k = 0.
__device__ __forceinline__ void poisson_ylogy_table(double* tab, int k) {
  const double y = (double)k;
  tab[k] = y > 0.0 ? y * log(y) : 0.0;
}
// w, w*z from the init constants c (init_const), the deviance and the statistics constant from
// the table; false: the row is not a tabulated count (caller takes the reference path)
__device__ __forceinline__ bool poisson_init_row(const double* c, const double* tab, double y, double off, double pw,
                                                 double& w, double& wz, double& s_dev, double& s_aux, double& s_lg) {
  if (!(y >= 0.0 && y < (double)POIS_TAB && y == floor(y))) return false;
  const int k = (int)y;
  w = pw * c[3];
  const double z = (c[0] + ((y + (-1.0 * c[1])) * c[2])) + (-1.0 * off);
  wz = w * z;
  s_dev += pw * tab[k];
  s_aux += pw;
  s_lg += pw * tab[POIS_TAB + k];
  return true;
}

// Per-row diagnostics at eta (influence.hip): the pass's working weight w = pw / (V g'^2)
// (row_core's, 0 where pw = 0), the Pearson residual (y - mu) sqrt(pw / V) that Cook's
// distance needs, and the residual of the requested type on the engine's count scale
// (mu = unlink(eta, m)): response y - mu, working (y - mu) g'(mu), Pearson, or deviance
// sign(y - mu) sqrt(factor * unit_dev) with the family factor the host applies to the deviance sum
// (driver.cpp family_dev_factor).  Reference-order functions only; out of line like pass_row_ref.
// The sandwich estimator's score weight (influence.hip score_kernel) is built on the same call: with
// RESID_WORKING, u = w * resid = w (y - mu) g'(mu) is the row's score contribution per unit of x.
enum ResidType : int { RESID_RESPONSE = 0, RESID_WORKING = 1, RESID_PEARSON = 2, RESID_DEVIANCE = 3 };
struct InflRow {
  double w, rp, resid;
};
__device__ __noinline__ InflRow influence_row(int fam, int lnk, int rtype, double eta, double y, double m, double pw,
                                              double theta) {
  // (noncanonical_pair: the links selected by link -- every negative binomial pair)
  const RowCore c = row_core(noncanonical_pair(fam, lnk), fam == FAM_NEGBIN, fam, lnk, MODE_IRLS, eta, m, pw, 0.0, theta);
  const double mu = c.mu;
  const double e = y + (-1.0 * mu);
  InflRow r;
  r.w = c.w;
  r.rp = e * sqrt(pw / c.v);
  if (rtype == RESID_RESPONSE) {
    r.resid = e;
  } else if (rtype == RESID_WORKING) {
    r.resid = e * c.g;
  } else if (rtype == RESID_PEARSON) {
    r.resid = r.rp;
  } else {
    const double d = fam == FAM_NEGBIN ? 2.0 * nb_unit_dev(y, mu, pw, theta)
                                       : (fam == FAM_GAUSSIAN ? 1.0 : 2.0) * unit_dev(fam, y, mu, m, pw);
    const double s = sqrt(fmax(d, 0.0));
    r.resid = e > 0.0 ? s : (e < 0.0 ? -s : 0.0);
  }
  return r;
}

// The row of Firth's adjusted score (influence.hip firth_kernel): the working weight w, the
// score u = w (y - mu) g'(mu) (the INFL_USCORE value) and r = d' / d with d = dmu / deta, d' = d2mu / deta2 -- the
// binomial's m cancels in r -- so that the row's adjustment is h r / 2, h = w q.  phi = 1 families only (binomial,
// poisson).  Reference-order functions; out of line like influence_row.
struct FirthRow {
  double w, u, r;
};
__device__ __noinline__ FirthRow firth_row(int fam, int lnk, double eta, double y, double m, double pw) {
  const RowCore c = row_core(noncanonical_pair(fam, lnk), CT<false>{}, fam, lnk, MODE_IRLS, eta, m, pw, 0.0, 0.0);
  FirthRow f;
  f.w = c.w;
  f.u = c.w * ((y + (-1.0 * c.mu)) * c.g);
  if (lnk == LNK_LOGIT) f.r = 1.0 - 2.0 * (c.mu / m);
  else if (lnk == LNK_PROBIT) f.r = -eta;
  else if (lnk == LNK_CLOGLOG) f.r = 1.0 - exp(eta);
  else if (lnk == LNK_LOG) f.r = 1.0;
  else if (lnk == LNK_SQRT) f.r = 1.0 / eta;
  else f.r = 0.0;
  return f;
}

#undef SGLM_LOGIT_FAST
#undef SGLM_POISSON_LOG_FAST
#undef SGLM_GAMMA_INVERSE_FAST

}  // namespace sglm
