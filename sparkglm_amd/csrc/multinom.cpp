// multinom.cpp -- multinomial logit fits (softmax regression; sglm_fit_multinom, sglm_multinom_pass; nnet::multinom,
// Stata mlogit, statsmodels MNLogit).
//
// y holds the class code 0 .. K - 1 of each row, class 0 is the baseline, B [p x (K - 1)] col-major: the parameter
// vector of length q = (K - 1) p is class-major.  One evaluation at B: the row kernel over every resident shard
// (multinom.hip: the deviance D = -2 sum pw log pi_y, the weighted class counts, and in the full mode P and the
// score g = vec(X'R) in one read of X, two past the fused shapes), summed over shards in order and over ranks by
// the small all-reduce.  The Hessian H = sum_i (diag(pi_i) - pi_i pi_i') (x) x_i x_i' is K (K - 1) / 2 symmetric
// p x p blocks X' diag(omega) X: for each pair the weight kernel writes omega into the shard's score weights and the
// tuned Gram pass runs under the meat-pass scope, as the sandwich covariance's meat does; the off-diagonal blocks'
// weights are pw pi_j pi_k >= 0 and the block is negated here.  The fit is Newton's method with step halving on
// the deviance (deviance-only evaluations) and R's glm.control stop rule.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.hpp"

using namespace sglm;

void sglm_engine::free_multinom() {
  dev_free({&dmnP, &dmnR, &dmnB, &dmnpart});
  mnP_cap = mnR_cap = mnpart_cap = 0;
  for (hipEvent_t& e : evmn) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

int sglm_engine::multinom_enqueue(int K, const double* B, int mode) {
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  for (hipEvent_t& e : evmn)
    if (!e) HIPCHK(hipEventCreate(&e));
  const int64_t q = (int64_t)(K - 1) * p;
  const int P = (int)((p + 15) / 16);
  const int grid = multinom_grid(ncu, n);
  // sized for the full mode: the deviance-only evaluations of a fit keep the buffer
  if (int rc = grow(dmnpart, mnpart_cap, (int64_t)(grid + 1) * (q + MN_NSC), "hipMalloc(multinomial partials)")) return rc;
  if (!dmnB)
    if (int rc = dev_alloc(&dmnB, sizeof(double) * MN_MAX_Q, "hipMalloc(multinomial coefficients)")) return rc;
  MultinomArgs a{};
  a.X = dX;
  a.ld = n_pad;
  a.p = (int)p;
  a.K = K;
  a.n = n;
  a.B = dmnB;
  a.y = dy;
  a.prior = dprior;
  a.part = dmnpart;
  a.nscore = mode == MN_FULL ? (int)q : 0;
  a.stride = a.nscore + MN_NSC;
  if (mode == MN_FULL) {
    if (int rc = grow(dmnP, mnP_cap, (int64_t)K * n_pad, "hipMalloc(multinomial probabilities)")) return rc;
    mn_two = !multinom_is_fused(P, K);
    if (mn_two)
      if (int rc = grow(dmnR, mnR_cap, (int64_t)(K - 1) * n_pad, "hipMalloc(multinomial residuals)")) return rc;
    a.P = dmnP;
    a.R = dmnR;
  }
  HIPCHK(hipMemcpyAsync(dmnB, B, sizeof(double) * (size_t)q, hipMemcpyHostToDevice, st));
  double* sum = dmnpart + (int64_t)grid * a.stride;
  if (n > 0) {
    HIPCHK(launch_multinom_rows(mode, P, a, grid, st, evmn[0], evmn[1], evmn[2]));
    HIPCHK(launch_part_sum(dmnpart, grid, a.stride, a.stride, sum, st));
  } else {
    HIPCHK(hipEventRecord(evmn[0], st));
    HIPCHK(hipEventRecord(evmn[1], st));
    HIPCHK(hipEventRecord(evmn[2], st));
    HIPCHK(hipMemsetAsync(sum, 0, sizeof(double) * (size_t)a.stride, st));
  }
  return SGLM_OK;
}

int sglm_engine::multinom_collect(int K, int mode, double* out, double* prob, int64_t ldp) {
  HIPCHK(hipSetDevice(device));
  const int64_t q = (int64_t)(K - 1) * p;
  const int64_t stride = (mode == MN_FULL ? q : 0) + MN_NSC;
  const int grid = multinom_grid(ncu, n);
  HIPCHK(hipMemcpyAsync(out, dmnpart + (int64_t)grid * stride, sizeof(double) * (size_t)stride, hipMemcpyDeviceToHost, st));
  if (prob && mode == MN_FULL)
    for (int j = 0; j < K && n > 0; ++j)
      HIPCHK(hipMemcpyAsync(prob + (int64_t)j * ldp, dmnP + (int64_t)j * n_pad, sizeof(double) * (size_t)n,
                            hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, evmn[0], evmn[1]));
  mn_ms[0] = t;
  mn_ms[1] = 0.0;
  if (mode == MN_FULL && mn_two && n > 0) {
    HIPCHK(hipEventElapsedTime(&t, evmn[1], evmn[2]));
    mn_ms[1] = t;
  }
  return SGLM_OK;
}

int sglm_engine::multinom_weight_local(int K, int j, int k) {
  HIPCHK(hipSetDevice(device));
  if (int rc = grow(domega, omega_cap, n_pad, "hipMalloc(score weights)")) return rc;
  if (n_pad > 0) {
    HIPCHK(launch_multinom_weight(dmnP, dprior, n, n_pad, K, j, k, domega, st, evmn[3], evmn[4]));
  } else {
    HIPCHK(hipEventRecord(evmn[3], st));
    HIPCHK(hipEventRecord(evmn[4], st));
  }
  return SGLM_OK;
}

namespace {

int mn_check_k(int K) {
  if (K < 2 || K > MN_MAX_K) {
    set_error("requirement failed: 2 <= n_classes <= " + std::to_string(MN_MAX_K) + " (got " + std::to_string(K) + ")");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

// what the handle must be, before any device call
int mn_check_handle(sglm_engine* h, int K) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = require_fused_or_narrow(h, "a multinomial fit needs")) return rc;
  if ((int64_t)(K - 1) * h->ncols() > MN_MAX_Q) {
    set_error("requirement failed: (n_classes - 1) * p <= " + std::to_string(MN_MAX_Q) + " (got " +
              std::to_string((int64_t)(K - 1) * h->ncols()) + ")");
    return SGLM_EINVAL;
  }
  for (const sglm_engine* s : h->shards())
    if (s->dm || s->doff) {
      set_error("requirement failed: a multinomial fit takes no trials m and no offset (prior weights are supported)");
      return SGLM_EINVAL;
    }
  return SGLM_OK;
}

// One evaluation at B: out [nscore + MN_NSC] over every shard and rank; prob: this handle's rows (a group: every
// shard's, in row order) [n x K] col-major, or null
int mn_eval(sglm_engine* h, int K, const double* B, int mode, std::vector<double>& out, double* prob) {
  const int64_t q = (int64_t)(K - 1) * h->ncols();
  const int64_t len = (mode == MN_FULL ? q : 0) + MN_NSC;
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards)
    if (int rc = s->multinom_enqueue(K, B, mode)) return rc;
  out.assign((size_t)len, 0.0);
  std::vector<double> part((size_t)len);
  const int64_t ldp = h->group() ? h->g_n : h->n;
  for (size_t d = 0; d < shards.size(); ++d) {
    const int64_t lo = h->group() ? h->sub_lo[d] : 0;
    if (int rc = shards[d]->multinom_collect(K, mode, part.data(), prob ? prob + lo : nullptr, ldp)) return rc;
    for (int64_t k = 0; k < len; ++k) out[(size_t)k] += part[(size_t)k];
  }
  h->mn_ms[0] = slowest_shard(h, [](const sglm_engine* s) { return s->mn_ms[0]; });
  h->mn_ms[1] = slowest_shard(h, [](const sglm_engine* s) { return s->mn_ms[1]; });
  if (!h->group())
    if (int rc = h->allreduce_small(out.data(), len)) return rc;
  const double* sc = out.data() + (len - MN_NSC);
  if (sc[MN_BAD] > 0.0) {
    set_error("requirement failed: y is an integer class code in 0 .. n_classes - 1 on every row of positive weight (" +
              std::to_string((long long)sc[MN_BAD]) + " rows are not)");
    return SGLM_EINVAL;
  }
  for (int k = 0; k < K; ++k)
    if (!(sc[MN_COUNT + k] > 0.0)) {
      set_error("requirement failed: every class has positive total weight (class " + std::to_string(k) + " has none)");
      return SGLM_EINVAL;
    }
  return SGLM_OK;
}

double mn_deviance(const std::vector<double>& out) { return -2.0 * out[out.size() - MN_NSC + MN_LL]; }

// H [q x q] col-major at the P of the last full evaluation: a Gram pass per block pair (collective)
int mn_hessian(sglm_engine* h, int K, double* H) {
  const int64_t p = h->ncols(), q = (int64_t)(K - 1) * p;
  std::vector<double> packed((size_t)packed_len(p)), zero((size_t)p, 0.0), M((size_t)(p * p)), x((size_t)p);
  double wms = 0.0, gms = 0.0;
  for (int j = 1; j < K; ++j)
    for (int k = j; k < K; ++k) {
      for (sglm_engine* s : h->shards())
        if (int rc = s->multinom_weight_local(K, j, k)) return rc;
      {
        MeatPassScope scope(h);
        if (int rc = h->pass(MODE_IRLS, zero.data(), 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, packed.data())) return rc;
      }
      // (the pass drained every shard's stream: the weight kernel's events before it are complete)
      double w = 0.0;
      for (sglm_engine* s : h->shards()) {
        HIPCHK(hipSetDevice(s->device));
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, s->evmn[3], s->evmn[4]));
        w = std::max(w, (double)t);
      }
      wms += w;
      gms += slowest_shard(h, [](const sglm_engine* s) { return s->last_pass_ms; });
      unpack_gram(packed.data(), p, M.data(), x.data());
      const double sign = j == k ? 1.0 : -1.0;
      for (int64_t b = 0; b < p; ++b)
        for (int64_t a = 0; a < p; ++a) {
          const double v = sign * M[(size_t)(a + b * p)];
          H[((j - 1) * p + a) + ((k - 1) * p + b) * q] = v;
          H[((k - 1) * p + b) + ((j - 1) * p + a) * q] = v;
        }
    }
  h->mn_ms[2] = wms;
  h->mn_ms[3] = gms;
  return SGLM_OK;
}

const char* MN_SINGULAR = "breeze.linalg.MatrixSingularException: the multinomial Hessian is singular";

// delta = solve(H, g) by the fit's solve rule, and (cov != null) inv(H)
int mn_solve(sglm_engine* h, int64_t q, const double* H, const double* g, double* delta, double* cov) {
  std::vector<double> packed((size_t)packed_len(q), 0.0);
  for (int64_t i = 0; i < q; ++i)
    for (int64_t j = 0; j <= i; ++j) packed[(size_t)(i * (i + 1) / 2 + j)] = H[i + j * q];
  std::memcpy(packed.data() + tri_count(q), g, sizeof(double) * (size_t)q);
  std::unique_ptr<SolverIface> solver = h->make_solver(q);
  const double t0 = now_ms();
  if (const int srv = solver->solve(packed.data(), delta)) {
    if (srv == SGLM_ESINGULAR) set_error(MN_SINGULAR);
    return srv;
  }
  if (cov)
    if (int rc = solver->inverse(cov)) return rc;
  h->solve_ms += now_ms() - t0;
  h->solve_path = solver->path();
  return SGLM_OK;
}

double mn_null_deviance(const double* sc, int K) {
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += sc[MN_COUNT + k] * std::log(sc[MN_COUNT + k] / sc[MN_SUMW]);
  return -2.0 * s;
}

}  // namespace

extern "C" {

int sglm_multinom_pass(sglm_engine* h, int n_classes, const double* B, double* H, double* g, double* scalars3,
                       double* prob) {
  if (int rc = mn_check_k(n_classes)) return rc;
  if (!B) {
    set_error("requirement failed: B");
    return SGLM_EINVAL;
  }
  if (int rc = mn_check_handle(h, n_classes)) return rc;
  const int K = n_classes;
  const int64_t q = (int64_t)(K - 1) * h->ncols();
  const int mode = H || g || prob ? MN_FULL : MN_DEV;
  std::vector<double> out;
  if (int rc = mn_eval(h, K, B, mode, out, prob)) return rc;
  const double* sc = out.data() + (out.size() - MN_NSC);
  if (g) std::memcpy(g, out.data(), sizeof(double) * (size_t)q);
  if (scalars3) {
    scalars3[0] = mn_deviance(out);
    scalars3[1] = sc[MN_SUMW];
    scalars3[2] = mn_null_deviance(sc, K);
  }
  if (H)
    if (int rc = mn_hessian(h, K, H)) return rc;
  return SGLM_OK;
}

int sglm_fit_multinom(sglm_engine* h, const sglm_multinom_opts* opts, const double* B_start, double* B,
                      double* std_err, double* cov, sglm_multinom_info* info) {
  if (!opts) {
    set_error("requirement failed: opts");
    return SGLM_EINVAL;
  }
  if (int rc = mn_check_k(opts->n_classes)) return rc;
  if (!(std::isfinite(opts->epsilon) && opts->epsilon > 0.0)) {
    set_error("requirement failed: epsilon is finite and > 0 (got " + std::to_string(opts->epsilon) + ")");
    return SGLM_EINVAL;
  }
  if (opts->max_iter < 0 || opts->max_halvings < 0) {
    set_error("requirement failed: max_iter >= 0, max_halvings >= 0");
    return SGLM_EINVAL;
  }
  if (!B) {
    set_error("requirement failed: B");
    return SGLM_EINVAL;
  }
  if (int rc = mn_check_handle(h, opts->n_classes)) return rc;
  const int K = opts->n_classes;
  const double eps = opts->epsilon;
  const int64_t q = (int64_t)(K - 1) * h->ncols();
  std::vector<double> beta((size_t)q, 0.0), trial((size_t)q), delta((size_t)q), H((size_t)(q * q)), C((size_t)(q * q));
  if (B_start) std::memcpy(beta.data(), B_start, sizeof(double) * (size_t)q);
  std::vector<double> cur, next;
  if (int rc = mn_eval(h, K, beta.data(), MN_FULL, cur, nullptr)) return rc;
  int iter = 0, halvings = 0, converged = 0;
  while (iter < opts->max_iter) {
    if (int rc = mn_hessian(h, K, H.data())) return rc;
    if (int rc = mn_solve(h, q, H.data(), cur.data(), delta.data(), nullptr)) return rc;
    // B + t delta, t = 1, 1/2, ...: accepted unless the deviance grows by more than the stop rule resolves
    const double d_old = mn_deviance(cur);
    double t = 1.0, d_new = d_old;
    bool accepted = false;
    for (int hv = 0;; ++hv) {
      for (int64_t i = 0; i < q; ++i) trial[(size_t)i] = beta[(size_t)i] + t * delta[(size_t)i];
      if (int rc = mn_eval(h, K, trial.data(), MN_DEV, next, nullptr)) return rc;
      d_new = mn_deviance(next);
      if (d_new - d_old <= eps * (std::fabs(d_new) + 0.1)) {
        accepted = true;
        break;
      }
      if (hv >= opts->max_halvings) break;
      t *= 0.5;
      halvings += 1;
    }
    if (!accepted) break;  // the search is abandoned: the fit stays at beta, not converged
    beta.swap(trial);
    iter += 1;
    if (int rc = mn_eval(h, K, beta.data(), MN_FULL, cur, nullptr)) return rc;
    if (std::fabs(d_old - d_new) / (std::fabs(d_new) + 0.1) < eps) {
      converged = 1;
      break;
    }
  }
  // everything returned is evaluated at the returned coefficients
  if (int rc = mn_hessian(h, K, H.data())) return rc;
  if (int rc = mn_solve(h, q, H.data(), cur.data(), delta.data(), C.data())) return rc;
  std::memcpy(B, beta.data(), sizeof(double) * (size_t)q);
  if (std_err)
    for (int64_t i = 0; i < q; ++i) std_err[i] = std::sqrt(C[(size_t)(i + i * q)]);
  if (cov) std::memcpy(cov, C.data(), sizeof(double) * C.size());
  if (info) {
    const double* sc = cur.data() + q;
    info->iter = iter;
    info->halvings = halvings;
    info->converged = converged;
    info->deviance = mn_deviance(cur);
    info->null_deviance = mn_null_deviance(sc, K);
    info->loglik = -0.5 * info->deviance;
    info->aic = info->deviance + 2.0 * (double)q;
    double si = 0.0;
    for (int64_t i = 0; i < q; ++i) {
      const double a = std::fabs(cur[(size_t)i]);
      si = (a > si || std::isnan(a)) ? a : si;
    }
    info->score_inf = si;
    for (int k = 0; k < MN_MAX_K; ++k) info->class_weight[k] = k < K ? sc[MN_COUNT + k] : 0.0;
  }
  return SGLM_OK;
}

int sglm_get_multinom_ms(sglm_engine* h, double* rows_ms, double* xtr_ms, double* weight_ms, double* gram_ms) {
  if (int rc = check_handle(h)) return rc;
  if (!rows_ms || !xtr_ms || !weight_ms || !gram_ms) {
    set_error("requirement failed: rows_ms, xtr_ms, weight_ms, gram_ms");
    return SGLM_EINVAL;
  }
  *rows_ms = h->mn_ms[0];
  *xtr_ms = h->mn_ms[1];
  *weight_ms = h->mn_ms[2];
  *gram_ms = h->mn_ms[3];
  return SGLM_OK;
}

}  // extern "C"
