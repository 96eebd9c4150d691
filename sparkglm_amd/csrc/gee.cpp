// gee.cpp -- GEE fits with an exchangeable working correlation over the cluster factor (sglm_fit_glm_gee,
// sglm_gee_pass, sglm_vcov_gee; Liang & Zeger; geepack::geeglm(corstr = "exchangeable")).
//
// With d = sqrt(w), R_g = (1 - rho) I + rho 11' and inv(R_g) = (I - c_g 11') / (1 - rho), c_g = rho / (1 - rho +
// n_g rho), one step's normal equations are A = (X'WX - sum c_g s_g s_g') / (1 - rho) and b = (X'Wz - sum c_g s_g
// t_g) / (1 - rho): the fixed-effects downdate (fe.cpp) with sqrt(w) for w and c_g for 1 / W_g.  One step at beta:
// an ordinary pass that stores eta; d and the per-segment sums of d z, 1[pw > 0], e, e^2 (gee_rows_kernel); the
// segment sums of d x (segment_sum_kernel); both through the combine tree into one buffer s | t | n | E | Q, summed
// over shards and ranks in one all-reduce; the five moments of that buffer (gee_moments_kernel) and from them
// rho(beta) and phi(beta) on the host; rows scaled by sqrt(|c_g|) (gee_scale_kernel) into the internal engine,
// whose LM Gram pass returns sum |c| s s' and sum |c| s t; the downdate with sign(rho) on the host.  The fit is
// glm_drive over a Backend whose pass is this step.  The step's frame, the bread and the finish of a clustered
// covariance are fe.cpp's and vcov_cluster.cpp's.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.hpp"

using namespace sglm;

void sglm_engine::free_gee() {
  dev_free({&dgm});
  free_group(gee);
}

// The buffers of a GEE step on this shard
int sglm_engine::gee_prepare() {
  if (int rc = group_prepare(gee)) return rc;
  if (!dgm)
    if (int rc = dev_alloc(&dgm, sizeof(double) * (size_t)((GEE_MOMENT_BLOCKS + 1) * NS), "hipMalloc(moment partials)"))
      return rc;
  return SGLM_OK;
}

// d (GEE_SCORE: d e) into domega at the rows' own offset, and the sums of d x (d e x), t | n | E | Q into gee.g
int sglm_engine::gee_sums_local(int kind, int mode, int family, int link, double mu0) {
  return group_sums_local(gee, launch_gee_rows, kind != GEE_COUNT, kind, mode, family, link, mu0, doff, nullptr, nullptr);
}

namespace {

// what the caller asked for, and what the last step found
struct GeeState {
  bool exch = true, fixed = false;
  double rho = 0.0;       // the fixed value
  double rho_used = 0.0;  // of the last step
  double m[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the moments of the last step (common.hpp GeeMoment)
};

int gee_read_opts(const sglm_gee_opts* gee, GeeState* g) {
  if (!gee) return SGLM_OK;
  if (gee->corstr != SGLM_COR_INDEPENDENCE && gee->corstr != SGLM_COR_EXCHANGEABLE) {
    set_error("requirement failed: corstr SGLM_COR_INDEPENDENCE or SGLM_COR_EXCHANGEABLE (got " +
              std::to_string(gee->corstr) + ")");
    return SGLM_EINVAL;
  }
  g->exch = gee->corstr == SGLM_COR_EXCHANGEABLE;
  g->fixed = g->exch && gee->fix_rho != 0;
  g->rho = g->fixed ? gee->rho : 0.0;
  if (g->fixed && !(std::isfinite(g->rho) && g->rho < 1.0)) {
    set_error("requirement failed: a fixed rho is finite and below 1 (got " + std::to_string(gee->rho) + ")");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

bool rho_valid(double rho, double n_max) { return rho < 1.0 && (1.0 - rho) + n_max * rho > 0.0; }

int rho_error(const char* what, double rho, double n_max, int iter) {
  set_error(std::string("requirement failed: ") + what + " rho = " + std::to_string(rho) + " is outside the range of "
            "a valid exchangeable correlation, rho < 1 and 1 - rho + n_max rho > 0 with n_max = " +
            std::to_string((int64_t)n_max) + (iter >= 0 ? " (iteration " + std::to_string(iter) + ")" : ""));
  return SGLM_EINVAL;
}

// The group sums of `kind` over every shard and rank: shard 0 of every rank ends with bitwise the same gee.g
int gee_group_sums(sglm_engine* h, int kind, int mode, int family, int link, double mu0) {
  for (sglm_engine* s : h->shards())
    if (int rc = s->gee_sums_local(kind, mode, family, link, mu0)) return rc;
  return group_sums_finish(h, &sglm_engine::gee, kind != GEE_COUNT);
}

// The moments of shard 0's all-reduced group buffer: NS doubles to the host, no G-sized download
int gee_moments(sglm_engine* h, double* m) {
  sglm_engine* s0 = h->shards()[0];
  HIPCHK(hipSetDevice(s0->device));
  GroupArgs a{};
  a.grp = s0->gee.g;
  a.G = s0->cl_G;
  a.ld = s0->cl_inner->n_pad;
  a.p = (int)s0->p;
  a.partials = s0->dgm;
  double* out = s0->dgm + (int64_t)GEE_MOMENT_BLOCKS * NS;
  HIPCHK(launch_gee_moments(a, out, s0->st));
  HIPCHK(hipMemcpyAsync(m, out, sizeof(double) * NS, hipMemcpyDeviceToHost, s0->st));
  HIPCHK(hipStreamSynchronize(s0->st));
  return SGLM_OK;
}

double phi_of(const double* m, int64_t p) { return m[M_Q] / (m[M_N] - (double)p); }
double rho_of(const double* m, int64_t p) {
  return (0.5 * (m[M_E2] - m[M_Q])) / ((m[M_PAIRS] - (double)p) * phi_of(m, p));
}

// The refusals that need the row counts, before the first pass: one launch of the rows kernel that reads the
// prior weights alone
int gee_counts(sglm_engine* h, const sglm_glm_opts* opts, GeeState* g) {
  const int64_t p = h->ncols();
  if (int rc = gee_group_sums(h, GEE_COUNT, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  if (int rc = gee_moments(h, g->m)) return rc;
  if (!(g->m[M_N] > (double)p)) {  // phi = sum Q / (N - p)
    set_error("requirement failed: more rows of positive prior weight, N = " + std::to_string((int64_t)g->m[M_N]) +
              ", than the p = " + std::to_string(p) + " columns");
    return SGLM_EINVAL;
  }
  if (!(g->m[M_PAIRS] > (double)p)) {  // rho's denominator
    set_error("requirement failed: more within-cluster pairs of rows, sum n_g (n_g - 1) / 2 = " +
              std::to_string((int64_t)g->m[M_PAIRS]) + ", than the p = " + std::to_string(p) + " columns");
    return SGLM_EINVAL;
  }
  if (g->fixed && !rho_valid(g->rho, g->m[M_NMAX])) return rho_error("the fixed", g->rho, g->m[M_NMAX], -1);
  return SGLM_OK;
}

// One step: packed = lower tri A | b | the pass's scalars, all-reduced; g->rho_used and g->m of this step.
// sums: form the group sums and the moments even where the step does not need them (the initial mode and
// independence, whose A and b are the pass's own).  iter: named by the refusal of an invalid estimate.
int gee_step(sglm_engine* h, int family, int link, int mode, const double* beta, double mu0, GeeState* g, bool sums,
             int iter, double* packed) {
  const int64_t p = h->ncols();
  if (int rc = h->pass(mode, beta, mu0, 0.0, family, link, packed)) return rc;
  const bool down = g->exch && mode == MODE_IRLS;
  g->rho_used = 0.0;
  if (!down && !sums) return SGLM_OK;
  if (int rc = gee_group_sums(h, GEE_STEP, mode, family, link, mu0)) return rc;
  if (int rc = gee_moments(h, g->m)) return rc;
  if (!down) return SGLM_OK;
  const double rho = g->fixed ? g->rho : rho_of(g->m, p);
  if (!rho_valid(rho, g->m[M_NMAX])) return rho_error(g->fixed ? "the fixed" : "the estimated", rho, g->m[M_NMAX], iter);
  g->rho_used = rho;
  if (rho == 0.0) return SGLM_OK;
  std::vector<double> dn((size_t)packed_len(p));
  if (int rc = group_gram(h, &sglm_engine::gee, launch_gee_scale, false, rho, dn.data())) return rc;
  const double omr = 1.0 - rho;
  if (rho > 0.0)
    for (int64_t k = 0; k < tri_count(p) + p; ++k) packed[k] = (packed[k] - dn[(size_t)k]) / omr;
  else
    for (int64_t k = 0; k < tri_count(p) + p; ++k) packed[k] = (packed[k] + dn[(size_t)k]) / omr;
  return SGLM_OK;
}

// The fit's Backend: glm_drive's pass is the GEE step; no deviance-only passes, no in-pass statistics (the
// passes store eta for the rows kernel).
struct GeeBackend : public StepBackend {
  GeeState* g;
  int iter = 0;
  GeeBackend(sglm_engine* handle, GeeState* state) : StepBackend(handle), g(state) {}
  int pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override {
    (void)ybar;
    if (mode == MODE_IRLS) iter += 1;
    return gee_step(h, family, link, mode, beta, mu0, g, false, iter, packed);
  }
};

const char* GEE_SINGULAR = "breeze.linalg.MatrixSingularException: the GEE step's X' inv(R) X is singular";

}  // namespace

extern "C" {

int sglm_fit_glm_gee(sglm_engine* h, const sglm_glm_opts* opts, const sglm_gee_opts* gee, sglm_preglm* out,
                     sglm_gee_info* info) {
  if (!out || !out->coefs || !out->std_err) {
    set_error("requirement failed: out, out->coefs, out->std_err");
    return SGLM_EINVAL;
  }
  GeeState g;
  if (int rc = gee_read_opts(gee, &g)) return rc;
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G, "a GEE fit needs", &sglm_engine::gee_prepare)) return rc;
  FeScope scope(h);
  if (int rc = gee_counts(h, opts, &g)) return rc;
  GeeBackend be(h, &g);
  if (int rc = drive_step_fit(be, *opts, out)) return rc;
  // rho and phi at the returned coefficients: one eta-storing pass without Gram, the rows kernel, the moments
  const int64_t p = h->ncols();
  std::vector<double> packed((size_t)packed_len(p));
  if (int rc = h->pass_dev(MODE_IRLS, out->coefs, 0.0, 0.0, opts->family, opts->link, packed.data())) return rc;
  if (int rc = gee_group_sums(h, GEE_STEP, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  if (int rc = gee_moments(h, g.m)) return rc;
  if (info) {
    info->rho = !g.exch ? 0.0 : g.fixed ? g.rho : rho_of(g.m, p);
    info->phi = phi_of(g.m, p);
    info->N = g.m[M_N];
    info->G_eff = (int32_t)g.m[M_GEFF];
    info->n_max = (int32_t)g.m[M_NMAX];
    info->rows_ms = h->gee.ms[0];
    info->sum_ms = h->gee.ms[1];
    info->combine_ms = h->gee.ms[2];
    info->gram_ms = h->gee.ms[3];
  }
  return SGLM_OK;
}

int sglm_gee_pass(sglm_engine* h, const sglm_glm_opts* opts, const sglm_gee_opts* gee, const double* beta, double* A,
                  double* b, double* group, double* moments, double* scalars, double* rho_used) {
  GeeState g;
  if (int rc = gee_read_opts(gee, &g)) return rc;
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G, "a GEE fit needs", &sglm_engine::gee_prepare)) return rc;
  FeScope scope(h);
  if (int rc = gee_counts(h, opts, &g)) return rc;
  const int64_t p = h->ncols();
  double mu0;
  int mode;
  if (int rc = fe_step_mode(h, opts, beta, &mode, &mu0)) return rc;
  std::vector<double> packed((size_t)packed_len(p));
  if (int rc = gee_step(h, opts->family, opts->link, mode, beta, mu0, &g, true, -1, packed.data())) return rc;
  fe_unpack_step(packed.data(), p, A, b, scalars);
  if (group) {
    sglm_engine* s0 = h->shards()[0];
    if (int rc = download_cols(s0, s0->gee.g, s0->cl_inner->n_pad, s0->cl_G, 0, p + GEE_NQ, group)) return rc;
  }
  if (moments) std::memcpy(moments, g.m, sizeof(double) * 5);
  if (rho_used) *rho_used = g.rho_used;
  return SGLM_OK;
}

int sglm_vcov_gee(sglm_engine* h, const sglm_glm_opts* opts, const sglm_gee_opts* gee, const double* beta, double rho,
                  int robust, int cadjust, double* cov, double* meat) {
  if (!beta || !cov) {
    set_error("requirement failed: beta, cov");
    return SGLM_EINVAL;
  }
  GeeState g;
  if (int rc = gee_read_opts(gee, &g)) return rc;
  // the covariance is formed at the rho it is given: a fixed one, whatever gee->fix_rho says
  g.fixed = g.exch;
  g.rho = g.exch ? rho : 0.0;
  if (g.exch && !(std::isfinite(rho) && rho < 1.0)) {
    set_error("requirement failed: rho is finite and below 1 (got " + std::to_string(rho) + ")");
    return SGLM_EINVAL;
  }
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G, "a GEE fit needs", &sglm_engine::gee_prepare)) return rc;
  if (robust)
    if (int rc = check_cadjust(cadjust, G)) return rc;
  FeScope scope(h);
  if (int rc = gee_counts(h, opts, &g)) return rc;
  const int64_t p = h->ncols();
  std::vector<double> packed((size_t)packed_len(p)), C((size_t)(p * p)), M((size_t)(p * p)), x((size_t)p);
  if (int rc = gee_step(h, opts->family, opts->link, MODE_IRLS, beta, 0.0, &g, true, -1, packed.data())) return rc;
  const double phi = phi_of(g.m, p);
  // a row whose working weight is not a number (its mean left the family's range) shows in the residual sums, and
  // from there in s, A, M and V alike: refused here, before a solve that would only call A singular
  if (!std::isfinite(g.m[M_E2]) || !std::isfinite(g.m[M_Q])) {
    set_error("requirement failed: the GEE covariance is not finite (a row whose mean leaves the family's range at "
              "beta)");
    return SGLM_EINVAL;
  }
  if (int rc = bread(h, packed.data(), GEE_SINGULAR, C.data())) return rc;
  if (!robust) {
    bool finite = std::isfinite(phi);
    for (size_t k = 0; k < C.size(); ++k) {
      cov[k] = phi * C[k];
      finite = finite && std::isfinite(cov[k]);
    }
    if (meat) std::fill(meat, meat + C.size(), 0.0);
    if (finite) return SGLM_OK;
    set_error("requirement failed: the model-based GEE covariance is not finite (a row whose mean leaves the "
              "family's range at beta)");
    return SGLM_EINVAL;
  }
  // the step's sums s | t | n | E | Q stay in g2 while the score-weighted ones S1 are formed in g
  if (int rc = h->shards()[0]->keep_group_sums(h->shards()[0]->gee)) return rc;
  if (int rc = gee_group_sums(h, GEE_SCORE, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  if (int rc = group_gram(h, &sglm_engine::gee, launch_gee_scale, true, g.rho, packed.data())) return rc;
  unpack_gram(packed.data(), p, M.data(), x.data());
  return clustered_finish(SGLM_HC0, 0.0, p, 0, G, cadjust, C, M, "beta", cov, meat);
}

int sglm_get_gee_ms(sglm_engine* h, double* ms) {
  if (int rc = check_handle(h)) return rc;
  if (!ms) {
    set_error("requirement failed: ms [4]");
    return SGLM_EINVAL;
  }
  std::memcpy(ms, h->gee.ms, sizeof(double) * 4);
  return SGLM_OK;
}

}  // extern "C"
