// firth.cpp -- Firth's bias-reduced fits of the phi = 1 families (sglm_fit_glm_firth, sglm_firth_pass; Firth 1993;
// Kosmidis & Firth 2009; logistf::logistf, brglm2::brglmFit(type = "AS_mean"), Stata firthlogit).
//
// The mean-bias-reducing adjusted score at beta, on the engine's scales (binomial mu = m pi, prior weights, offset):
//   g*(beta) = sum_i (u_i + h_i r_i / 2) x_i,  u_i = w_i (y_i - mu_i) g'(mu_i),  h_i = w_i x_i' C x_i,  C = inv(X'WX),
//   r = (d2mu / deta2) / (dmu / deta)   (logit 1 - 2 pi, probit -eta, cloglog 1 - e^eta, log 1, sqrt 1 / eta, identity 0)
// -- for the canonical links the gradient of l(beta) + log det(X'WX) / 2, the Jeffreys penalty.  One Firth pass at
// beta: the ordinary pass (A = X'WX, the deviance), C and log det A by the fit's solve rule, C~ to every shard, the
// Firth kernel over every resident shard (influence.hip: g* and sum h in one read of X, two past the fused widths),
// summed over shards in order and over ranks by the small all-reduce.  The fit is quasi-Fisher scoring, beta += C g*,
// with brglm2's step halving on |g*|_inf; g* is formed from u + a directly, not as X'Wz - X'WX beta.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "engine.hpp"

using namespace sglm;

namespace {

constexpr bool firth_pair(int fam, int lnk) {
  return (fam == FAM_BINOMIAL || fam == FAM_POISSON) && family_link_pair(fam, lnk);
}

// what every entry point requires of its arguments alone: before any device call and before the handle is looked at
int firth_check_opts(const sglm_glm_opts* opts, const sglm_firth_opts* fo) {
  if (!opts || !firth_pair(opts->family, opts->link)) {
    set_error("requirement failed: a Firth fit takes binomial (logit, probit, cloglog) or poisson (log, identity, "
              "sqrt); the families with a dispersion are not supported");
    return SGLM_EINVAL;
  }
  if (fo && !(std::isfinite(fo->epsilon) && fo->epsilon > 0.0)) {
    set_error("requirement failed: epsilon is finite and > 0 (got " + std::to_string(fo->epsilon) + ")");
    return SGLM_EINVAL;
  }
  if (fo && (fo->maxit < 0 || fo->max_halvings < 0)) {
    set_error("requirement failed: maxit >= 0, max_halvings >= 0");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

int firth_check_handle(sglm_engine* h) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  return require_fused_or_narrow(h, "a Firth fit needs");
}

// One Firth pass at beta and what the step from there needs
struct FirthEval {
  std::vector<double> packed, C, g, delta;  // lower tri A | X'Wz | scalars; inv(A); g* [p] | sum h; C g*
  double logdet = 0.0, score_inf = 0.0, delta_l1 = 0.0;
  explicit FirthEval(int64_t p)
      : packed((size_t)packed_len(p)), C((size_t)(p * p)), g((size_t)(p + 1)), delta((size_t)p) {}
  double sum_hat() const { return g.back(); }
};

const char* FIRTH_SINGULAR = "breeze.linalg.MatrixSingularException: X'WX is singular";

// hat: this handle's rows (a group: every shard's, in row order), or null
int firth_eval(sglm_engine* h, const sglm_glm_opts& o, const double* beta, FirthEval& e, double* hat) {
  const int64_t p = h->ncols();
  if (int rc = h->pass(MODE_IRLS, beta, 0.0, 0.0, o.family, o.link, e.packed.data())) return rc;
  if (int rc = bread(h, e.packed.data(), FIRTH_SINGULAR, e.C.data(), &e.logdet)) return rc;
  // shard order: g* and sum h summed as the shards lie, hat concatenated in row order; kernel time: the slowest shard
  const std::vector<sglm_engine*>& shards = h->shards();
  std::vector<double> part((size_t)(p + 1));
  std::fill(e.g.begin(), e.g.end(), 0.0);
  for (size_t d = 0; d < shards.size(); ++d) {
    const int64_t lo = h->group() ? h->sub_lo[d] : 0;
    if (int rc = shards[d]->firth_local(beta, e.C.data(), o.family, o.link, part.data(), hat ? hat + lo : nullptr))
      return rc;
    for (int64_t k = 0; k <= p; ++k) e.g[(size_t)k] += part[(size_t)k];
  }
  h->firth_ms = slowest_shard(h, [](const sglm_engine* s) { return s->firth_ms; });
  if (!h->group())
    if (int rc = h->allreduce_small(e.g.data(), p + 1)) return rc;
  e.score_inf = 0.0;
  e.delta_l1 = 0.0;
  for (int64_t i = 0; i < p; ++i) {
    const double a = std::fabs(e.g[(size_t)i]);
    e.score_inf = (a > e.score_inf || std::isnan(a)) ? a : e.score_inf;  // a NaN stays
    double s = 0.0;
    for (int64_t k = 0; k < p; ++k) s += e.C[(size_t)(i + k * p)] * e.g[(size_t)k];
    e.delta[(size_t)i] = s;
    e.delta_l1 += std::fabs(s);
  }
  return SGLM_OK;
}

double deviance_of(const FirthEval& e, int family, int64_t p) {
  return family_dev_factor(family) * e.packed[(size_t)(tri_count(p) + p + S_DEV)];
}

}  // namespace

extern "C" {

int sglm_fit_glm_firth(sglm_engine* h, const sglm_glm_opts* opts, const sglm_firth_opts* firth_opts,
                       const double* beta_start, sglm_preglm* out, sglm_firth_info* info) {
  if (int rc = firth_check_opts(opts, firth_opts)) return rc;
  if (!out || !out->coefs || !out->std_err) {
    set_error("requirement failed: out, out->coefs, out->std_err");
    return SGLM_EINVAL;
  }
  if (int rc = firth_check_handle(h)) return rc;
  const sglm_glm_opts& o = *opts;
  const double epsilon = firth_opts ? firth_opts->epsilon : 1e-8;
  const int maxit = firth_opts ? firth_opts->maxit : 100;
  const int max_halvings = firth_opts ? firth_opts->max_halvings : 12;
  const int64_t p = h->ncols();
  // the start: the engine's initial pass (the null deviance too) and, without beta_start, its solve -- sglm_fit_glm's
  // first iterate
  double sums[2];
  if (int rc = h->global_sums(sums)) return rc;
  const double nrow = sums[1];
  if (!(nrow > 0)) {
    set_error("requirement failed: The number of rows must be strictly greater than 0");
    return SGLM_EINVAL;
  }
  const double ymean = sums[0] / nrow;
  const int init_mode = o.init_mode == SGLM_INIT_MULTIPLE ? MODE_INIT_MULTI : MODE_INIT_SINGLE;
  std::vector<double> beta((size_t)p), trial((size_t)p), s(NS);
  FirthEval cur(p), next(p);
  if (int rc = h->pass(init_mode, nullptr, ymean, 0.0, o.family, o.link, cur.packed.data())) return rc;
  const double null_dev = deviance_of(cur, o.family, p);
  if (beta_start) {
    std::memcpy(beta.data(), beta_start, sizeof(double) * (size_t)p);
  } else {
    std::unique_ptr<SolverIface> solver = h->make_solver(p);
    const int srv = solver->solve(cur.packed.data(), beta.data());
    if (srv) {
      if (srv == SGLM_ESINGULAR) set_error(FIRTH_SINGULAR);
      return srv;
    }
  }
  if (int rc = firth_eval(h, o, beta.data(), cur, nullptr)) return rc;
  double pass_ms = 0.0;
  int iter = 0, halvings = 0, converged = 0;
  if (out->dev_trace && out->max_trace > 0) out->dev_trace[0] = deviance_of(cur, o.family, p);
  for (;;) {
    if (cur.delta_l1 < epsilon) {
      converged = 1;
      break;
    }
    if (iter >= maxit) break;
    // beta + delta, halved while the adjusted score there is not finite or larger than here (brglm2); past
    // max_halvings the last trial stands
    double f = 1.0;
    for (int hv = 0;; ++hv) {
      for (int64_t i = 0; i < p; ++i) trial[(size_t)i] = beta[(size_t)i] + f * cur.delta[(size_t)i];
      if (int rc = firth_eval(h, o, trial.data(), next, nullptr)) return rc;
      if ((std::isfinite(next.score_inf) && next.score_inf <= cur.score_inf) || hv >= max_halvings) break;
      f *= 0.5;
      halvings += 1;
    }
    beta.swap(trial);
    std::swap(cur, next);
    iter += 1;
    if (out->dev_trace && iter < out->max_trace) out->dev_trace[iter] = deviance_of(cur, o.family, p);
    if (o.verbose) {
      std::printf("%d\t%.17g\n", iter, cur.delta_l1);
      std::fflush(stdout);
    }
  }
  for (const sglm_engine* sh : h->shards()) pass_ms = std::max(pass_ms, sh->last_pass_ms);
  // the last pass was the one at the returned beta: its statistics, as glm_drive takes them
  if (h->pass_has_stats()) {
    std::memcpy(s.data(), cur.packed.data() + tri_count(p) + p, sizeof(double) * NS);
  } else if (int rc = h->stats(MODE_IRLS, beta.data(), ymean, 0.0, o.family, o.link, s.data())) {
    return rc;
  }
  if (s[S_BAD] > 0) {
    set_error("requirement failed: Binomial(m.toInt, mu).logProbabilityOf(y.toInt) needs 0 <= y <= m, m >= 1");
    return SGLM_EINVAL;
  }
  for (int64_t i = 0; i < p; ++i) {
    out->coefs[i] = beta[(size_t)i];
    out->std_err[i] = std::sqrt(cur.C[(size_t)(i + i * p)]);
  }
  out->deviance = deviance_of(cur, o.family, p);
  out->null_deviance = null_dev;
  out->pearson = s[S_PEARSON];
  out->loglik = s[S_LL];
  out->iter = iter;
  out->nrow = nrow;
  out->npart = o.npart > 0 ? o.npart : h->npart();
  if (info) {
    info->iterations = iter;
    info->converged = converged;
    info->halvings = halvings;
    info->deviance = out->deviance;
    info->pen_deviance = out->deviance - cur.logdet;
    info->logdet = cur.logdet;
    info->score_inf = cur.score_inf;
    info->sum_hat = cur.sum_hat();
    info->firth_ms = h->firth_ms;
    info->pass_ms = pass_ms;
  }
  return SGLM_OK;
}

int sglm_firth_pass(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double* A, double* g, double* hat,
                    double* scalars) {
  if (int rc = firth_check_opts(opts, nullptr)) return rc;
  if (!beta) {
    set_error("requirement failed: beta");
    return SGLM_EINVAL;
  }
  if (int rc = firth_check_handle(h)) return rc;
  const int64_t p = h->ncols();
  FirthEval e(p);
  if (int rc = firth_eval(h, *opts, beta, e, hat)) return rc;
  if (A) {
    std::vector<double> x((size_t)p);
    unpack_gram(e.packed.data(), p, A, x.data());
  }
  if (g) std::memcpy(g, e.g.data(), sizeof(double) * (size_t)p);
  if (scalars) {
    scalars[0] = deviance_of(e, opts->family, p);
    scalars[1] = e.logdet;
    scalars[2] = e.sum_hat();
  }
  return SGLM_OK;
}

int sglm_get_firth_ms(sglm_engine* h, double* ms) {
  if (int rc = check_handle(h)) return rc;
  if (!ms) {
    set_error("requirement failed: ms");
    return SGLM_EINVAL;
  }
  *ms = h->firth_ms;
  return SGLM_OK;
}

}  // extern "C"
