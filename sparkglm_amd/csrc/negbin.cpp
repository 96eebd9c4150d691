// negbin.cpp -- the negative binomial family on the host side (theta.hip): theta on the
// handle, the theta terms and their all-reduce, MASS::theta.ml's Newton iteration, the warm-started fit and
// MASS::glm.nb's alternation.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.hpp"

using namespace sglm;

int sglm_engine::theta_check(int family) const {
  if (family != FAM_NEGBIN || (theta > 0.0 && std::isfinite(theta))) return SGLM_OK;
  set_error("requirement failed: the negative binomial family needs theta: none was set on this handle "
            "(sglm_set_theta, or sglm_fit_glm_nb to estimate it)");
  return SGLM_EINVAL;
}

// this shard's sums into s[NS] (THETA_NT of them; the rest zero)
int sglm_engine::theta_terms_local(int link, double th, bool loglik, double* s) {
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  if (int rc = ensure_small(64)) return rc;
  if (!evt0) HIPCHK(hipEventCreate(&evt0));
  if (!evt1) HIPCHK(hipEventCreate(&evt1));
  ThetaArgs a{};
  a.y = dy;
  a.eta = deta;
  a.prior = dprior;
  a.n = n;
  a.link = link;
  a.theta = th;
  a.partials = dpart;
  const int nb = stats_blocks(n);  // the statistics pass's partial count (engine.hpp): within dpart
  HIPCHK(launch_theta_terms(a, nb, loglik, st, evt0, evt1));
  HIPCHK(launch_reduce_stats(dpart, nb, dsmall, st));
  HIPCHK(hipMemcpyAsync(hsmall, dsmall, sizeof(double) * NS, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, evt0, evt1));
  theta_ms += ms;
  theta_launches += 1;
  std::memcpy(s, hsmall, sizeof(double) * NS);
  return SGLM_OK;
}

int sglm_engine::theta_terms(int link, double th, bool loglik, double* out5) {
  double s[NS];
  if (group()) {  // shard order, compensated (as stats)
    std::vector<double> blocks((size_t)NS * subs.size());
    for (size_t d = 0; d < subs.size(); ++d)
      if (int rc = subs[d]->theta_terms_local(link, th, loglik, blocks.data() + NS * d)) return rc;
    compensated_rank_sum(blocks.data(), (int)subs.size(), NS, s);
    theta_launches += 1;
    theta_ms = 0.0;
    for (sglm_engine* sub : subs) theta_ms = std::max(theta_ms, sub->theta_ms);  // the slowest shard
  } else {
    if (int rc = theta_terms_local(link, th, loglik, s)) return rc;
    if (int rc = allreduce_small(s, NS)) return rc;
  }
  std::memcpy(out5, s, sizeof(double) * THETA_NT);
  return SGLM_OK;
}

namespace {

bool nb_link(int link) { return family_link_pair(FAM_NEGBIN, link); }

int bad_link() {
  set_error("requirement failed: the negative binomial's links are log, sqrt and identity");
  return SGLM_EINVAL;
}

void set_theta_all(sglm_engine* h, double th) {
  h->theta = th;
  for (sglm_engine* s : h->subs) s->theta = th;
}

// While it lives every IRLS pass of the handle's shards stores eta (no in-pass statistics).
struct EtaScope {
  sglm_engine* h;
  explicit EtaScope(sglm_engine* handle) : h(handle) {
    for (sglm_engine* s : h->shards()) s->want_eta = true;
  }
  ~EtaScope() {
    for (sglm_engine* s : h->shards()) s->want_eta = false;
  }
};

// eta = X beta + offset of every shard into its eta buffer: one deviance-only Poisson pass at the link (the
// pass kernels' own eta, no Gram; its scalars are not used -- a row outside the range is the theta terms' to
// report)
int form_eta(sglm_engine* h, int link, const double* beta) {
  EtaScope scope(h);
  std::vector<double> packed((size_t)packed_len(h->ncols()));
  return h->pass_dev(MODE_IRLS, beta, 0.0, 0.0, FAM_POISSON, link, packed.data());
}

struct ThetaMl {
  double theta = 0.0, se = 0.0;
  int iters = 0, warn = 0;
};

// MASS::theta.ml over the eta the shards hold
int theta_ml_run(sglm_engine* h, int link, int limit, double eps, ThetaMl* r) {
  if (limit <= 0) limit = 25;
  if (!(eps > 0.0)) eps = std::ldexp(1.0, -13);
  double t[THETA_NT];
  // the starting value needs no theta: the kernel runs at theta = 1 for its last two sums
  if (int rc = h->theta_terms(link, 1.0, false, t)) return rc;
  double t0 = t[T_SUMW] / t[T_MOM];
  double del = 1.0, info = NAN;
  int it = 0;
  while (++it < limit && std::fabs(del) > eps) {
    t0 = std::fabs(t0);
    if (!(t0 > 0.0) || !std::isfinite(t0)) break;  // nothing to evaluate at: reported below
    if (int rc = h->theta_terms(link, t0, false, t)) return rc;
    info = t[T_INFO];
    del = t[T_SCORE] / info;
    t0 = t0 + del;
  }
  if (!std::isfinite(t0) || !std::isfinite(del)) {
    set_error("requirement failed: theta.ml: the theta score is not finite (a row with mu <= 0 at beta, or a "
              "degenerate starting value sum w / sum w (y/mu - 1)^2)");
    return SGLM_EINVAL;
  }
  r->warn = 0;
  if (t0 < 0.0) {
    t0 = 0.0;
    r->warn |= 2;  // "estimate truncated at zero"
  }
  if (it == limit) r->warn |= 1;  // "iteration limit reached"
  r->theta = t0;
  r->se = std::sqrt(1.0 / info);
  r->iters = it;
  return SGLM_OK;
}

int check_fit_args(const sglm_glm_opts* opts, const sglm_preglm* out) {
  if (!opts || !out || !out->coefs || !out->std_err) {
    set_error("requirement failed: opts, out, out->coefs, out->std_err");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

}  // namespace

extern "C" {

int sglm_set_theta(sglm_engine* h, double theta) {
  if (!(theta > 0.0) || !std::isfinite(theta)) {
    set_error("requirement failed: theta > 0 and finite");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  set_theta_all(h, theta);
  return SGLM_OK;
}

int sglm_get_theta(sglm_engine* h, double* theta) {
  if (int rc = check_handle(h)) return rc;
  if (!theta) {
    set_error("requirement failed: theta");
    return SGLM_EINVAL;
  }
  *theta = h->theta;
  return SGLM_OK;
}

int sglm_get_theta_ms(sglm_engine* h, int64_t* launches, double* kernel_ms) {
  if (int rc = check_handle(h)) return rc;
  if (!launches || !kernel_ms) {
    set_error("requirement failed: launches, kernel_ms");
    return SGLM_EINVAL;
  }
  *launches = h->theta_launches;
  *kernel_ms = h->theta_ms;
  return SGLM_OK;
}

int sglm_nb_theta_terms(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double theta, double* out5) {
  if (!opts || !beta || !out5) {
    set_error("requirement failed: opts, beta, out");
    return SGLM_EINVAL;
  }
  if (!nb_link(opts->link)) return bad_link();
  if (!(theta > 0.0) || !std::isfinite(theta)) {
    set_error("requirement failed: theta > 0 and finite");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = form_eta(h, opts->link, beta)) return rc;
  return h->theta_terms(opts->link, theta, true, out5);
}

int sglm_theta_ml(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, int limit, double eps, double* theta,
                  double* se, int* iters, int* warn) {
  if (!opts || !beta || !theta) {
    set_error("requirement failed: opts, beta, theta");
    return SGLM_EINVAL;
  }
  if (!nb_link(opts->link)) return bad_link();
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = form_eta(h, opts->link, beta)) return rc;
  ThetaMl r;
  if (int rc = theta_ml_run(h, opts->link, limit, eps, &r)) return rc;
  *theta = r.theta;
  if (se) *se = r.se;
  if (iters) *iters = r.iters;
  if (warn) *warn = r.warn;
  return SGLM_OK;
}

int sglm_fit_glm_start(sglm_engine* h, const sglm_glm_opts* opts, const double* beta_start, sglm_preglm* out) {
  if (int rc = check_fit_args(opts, out)) return rc;
  if (!beta_start) {
    set_error("requirement failed: beta_start");
    return SGLM_EINVAL;
  }
  if (!family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: unsupported family/link combination");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  return glm_drive(*h, *opts, out, beta_start);
}

int sglm_fit_glm_nb(sglm_engine* h, const sglm_glm_opts* opts, const sglm_nb_opts* nbo, sglm_preglm* out,
                    sglm_nb_result* nb) {
  if (int rc = check_fit_args(opts, out)) return rc;
  if (!nb) {
    set_error("requirement failed: the sglm_nb_result");
    return SGLM_EINVAL;
  }
  if (!nb_link(opts->link)) return bad_link();
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  const int maxit = nbo && nbo->maxit > 0 ? nbo->maxit : 25;
  const double epsilon = nbo && nbo->epsilon > 0.0 ? nbo->epsilon : 1e-8;
  const int tlimit = nbo ? nbo->theta_limit : 0;
  const double teps = nbo ? nbo->theta_eps : 0.0;
  const int64_t p = h->ncols();
  const int link = opts->link;
  sglm_glm_opts o = *opts;
  std::vector<double> beta((size_t)p);
  ThetaMl tm;
  double t[THETA_NT];
  {  // the Poisson fit; every pass stores eta, so the theta kernel reads the fit's own
    EtaScope scope(h);
    o.family = FAM_POISSON;
    if (int rc = glm_drive(*h, o, out)) return rc;
  }
  // the canonical Poisson pair does not stop on a non-finite deviance (a negative or non-finite y): stop here,
  // before anything is estimated from such a fit
  if (!std::isfinite(out->deviance) || !std::isfinite(out->null_deviance)) {
    set_error("requirement failed: glm.nb: the Poisson fit's deviance is not finite (the counts y must be finite "
              "and >= 0, mu finite and > 0)");
    return SGLM_EINVAL;
  }
  if (out->iter == 0) {  // no IRLS pass ran (tol >= 1): no eta at the coefficients yet
    if (int rc = form_eta(h, link, out->coefs)) return rc;
  }
  std::memcpy(beta.data(), out->coefs, sizeof(double) * (size_t)p);
  if (int rc = theta_ml_run(h, link, tlimit, teps, &tm)) return rc;
  double theta = tm.theta;
  auto twologlik = [&](double th, double* lm) {
    if (!(th > 0.0)) {
      set_error("requirement failed: glm.nb: theta was truncated at zero (the counts are not overdispersed "
                "relative to the Poisson fit)");
      return (int)SGLM_EINVAL;
    }
    if (int rc = h->theta_terms(link, th, true, t)) return rc;
    *lm = 2.0 * t[T_LL];
    return (int)SGLM_OK;
  };
  double Lm = 0.0;
  if (int rc = twologlik(theta, &Lm)) return rc;
  const double d1 = std::sqrt(2.0 * std::max(1.0, out->nrow - (double)p));
  double del = 1.0, Lm0 = Lm + 2.0 * d1;
  int it = 0;
  o.family = FAM_NEGBIN;
  while ((it += 1) <= maxit && std::fabs(Lm0 - Lm) / d1 + std::fabs(del) > epsilon) {
    set_theta_all(h, theta);
    if (int rc = glm_drive(*h, o, out, beta.data())) return rc;  // its last pass stored eta at out->coefs
    std::memcpy(beta.data(), out->coefs, sizeof(double) * (size_t)p);
    const double t0 = theta;
    if (int rc = theta_ml_run(h, link, tlimit, teps, &tm)) return rc;
    theta = tm.theta;
    del = t0 - theta;
    Lm0 = Lm;
    if (int rc = twologlik(theta, &Lm)) return rc;
  }
  set_theta_all(h, theta);
  nb->outer_iter = it - 1;  // inner fits run
  nb->converged = it > maxit ? 0 : 1;
  if (nb->outer_iter > 0) {  // the null deviance at the final theta: one initial-mode pass at mean(y)
    std::vector<double> packed((size_t)packed_len(p));
    double sums[2];
    if (int rc = h->global_sums(sums)) return rc;
    const int init_mode = (o.init_mode == SGLM_INIT_MULTIPLE) ? MODE_INIT_MULTI : MODE_INIT_SINGLE;
    if (int rc = h->pass(init_mode, nullptr, sums[0] / sums[1], 0.0, FAM_NEGBIN, link, packed.data())) return rc;
    out->null_deviance = family_dev_factor(FAM_NEGBIN) * packed[(size_t)(tri_count(p) + p + S_DEV)];
  }
  out->loglik = Lm / 2.0;
  nb->theta = theta;
  nb->se_theta = tm.se;
  nb->twologlik = Lm;
  nb->theta_warn = tm.warn;
  return SGLM_OK;
}

}  // extern "C"
