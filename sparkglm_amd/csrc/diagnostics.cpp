// diagnostics.cpp -- what follows a fit (influence.hip): the covariance inv(X'WX) (sglm_vcov), the
// per-row diagnostics -- leverage, residuals, Cook's distance (sglm_influence) -- se.fit of new
// rows (sglm_predict_new_se) and the sandwich covariance HC0-HC3 (sglm_vcov_robust), with the
// host arithmetic of the sandwich.
#include <algorithm>
#include <cstring>

#include "engine.hpp"

using namespace sglm;

void sglm_engine::free_influence() {
  omega_cap = 0;
  dev_free({&dct, &dinf[0], &dinf[1], &dinf[2], &dhpart, &domega, &dgpart});
  gpart_cap = 0;
  if (hct) (void)hipHostFree(hct);
  hct = nullptr;
  inf_cap[0] = inf_cap[1] = inf_cap[2] = 0;
  hpart_cap = 0;
  if (evi0) (void)hipEventDestroy(evi0);
  if (evi1) (void)hipEventDestroy(evi1);
  evi0 = evi1 = nullptr;
}

// cov (col-major pp x pp) -> C~ tiles on the device
int sglm_engine::upload_cov(const double* cov, int64_t pp) {
  constexpr size_t CT_BYTES = sizeof(double) * (size_t)(MAX_P16 * (MAX_P16 + 1) / 2) * INFL_TILE;
  if (!dct)
    if (int rc = dev_alloc(&dct, CT_BYTES, "hipMalloc(covariance tiles)")) return rc;
  if (!hct) HIPCHK(hipHostMalloc(&hct, CT_BYTES, hipHostMallocDefault));
  const int64_t P = (pp + 15) / 16;
  influence_tiles(cov, (int)pp, hct);
  HIPCHK(hipMemcpyAsync(dct, hct, sizeof(double) * (size_t)(P * (P + 1) / 2) * INFL_TILE, hipMemcpyHostToDevice, st));
  return SGLM_OK;
}

// the row kernels' view of the resident shard at dbeta, into a
static void resident_args(const sglm_engine& e, int family, int link, InflArgs& a) {
  a.X = e.dX;
  a.ld = e.n_pad;
  a.p = (int)e.p;
  a.n = e.n;
  a.ct = e.dct;
  a.beta = e.dbeta;
  a.y = e.dy;
  a.m = e.dm;
  a.off = e.doff;
  a.prior = e.dprior;
  a.family = family;
  a.link = link;
  a.theta = e.theta;
}

int sglm_engine::rows_grid(int mode) const { return infl_grid(mode, (int)((p + 15) / 16), ncu, n); }

// The host frame of every launch of the row kernel over the resident shard (engine.hpp)
int sglm_engine::rows_enqueue(int mode, const double* beta, const double* cov, int family, int link, InflArgs a,
                              bool to_omega) {
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  if (!evi0) HIPCHK(hipEventCreate(&evi0));
  if (!evi1) HIPCHK(hipEventCreate(&evi1));
  if (to_omega)
    if (int rc = grow(domega, omega_cap, n_pad, "hipMalloc(score weights)")) return rc;
  if (cov)
    if (int rc = upload_cov(cov, p)) return rc;
  std::memcpy(hbeta, beta, sizeof(double) * p);
  HIPCHK(hipMemcpyAsync(dbeta, hbeta, sizeof(double) * p, hipMemcpyHostToDevice, st));
  resident_args(*this, family, link, a);
  a.need_q = cov ? 1 : 0;
  if (to_omega) {
    a.out = domega;
    // the padding rows of X are zero, but the pass multiplies them by their weight: 0, not what the
    // allocation held
    if (n_pad > n) HIPCHK(hipMemsetAsync(domega + n, 0, sizeof(double) * (size_t)(n_pad - n), st));
  }
  if (n > 0) {
    HIPCHK(launch_infl(mode, (int)((p + 15) / 16), a, rows_grid(mode), st, evi0, evi1));
  } else {
    HIPCHK(hipEventRecord(evi0, st));
    HIPCHK(hipEventRecord(evi1, st));
  }
  return SGLM_OK;
}

int sglm_engine::rows_sync(double* ms) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamSynchronize(st));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, evi0, evi1));
  *ms = t;
  return SGLM_OK;
}

// hat / resid / cooks / sum of h of this shard's rows at beta against cov (the global C); any output null
int sglm_engine::influence_local(const double* beta, const double* cov, int family, int link, int rtype, double disp,
                                 double* hat, double* resid, double* cooks, double* sum_hat) {
  HIPCHK(hipSetDevice(device));
  double* outs[3] = {hat, resid, cooks};
  for (int k = 0; k < 3; ++k)
    if (outs[k])
      if (int rc = grow(dinf[k], inf_cap[k], n_pad, "hipMalloc(diagnostics vector)")) return rc;
  const int g = rows_grid(INFL_ROWS);
  if (int rc = grow(dhpart, hpart_cap, g + 1, "hipMalloc(leverage partials)")) return rc;
  InflArgs a{};
  a.resid_type = rtype;
  a.dispersion = disp;
  a.hat = hat ? dinf[0] : nullptr;
  a.resid = resid ? dinf[1] : nullptr;
  a.cooks = cooks ? dinf[2] : nullptr;
  a.hpart = sum_hat ? dhpart : nullptr;
  if (int rc = rows_enqueue(INFL_ROWS, beta, hat || cooks || sum_hat ? cov : nullptr, family, link, a)) return rc;
  if (sum_hat) *sum_hat = 0.0;
  if (n > 0) {
    if (sum_hat) {
      HIPCHK(launch_infl_sum(dhpart, g, 1, dhpart + g, st));
      HIPCHK(hipMemcpyAsync(sum_hat, dhpart + g, sizeof(double), hipMemcpyDeviceToHost, st));
    }
    for (int k = 0; k < 3; ++k)
      if (outs[k]) HIPCHK(hipMemcpyAsync(outs[k], dinf[k], sizeof(double) * n, hipMemcpyDeviceToHost, st));
  }
  return rows_sync(&influence_ms);
}

// Firth's adjusted score of this shard's rows (firth.cpp): g = g* [p] | sum of h, the workgroups' partials added on
// the device in a fixed order; hat as influence_local's.  Past the fused widths v goes through domega.
int sglm_engine::firth_local(const double* beta, const double* cov, int family, int link, double* g, double* hat) {
  HIPCHK(hipSetDevice(device));
  std::fill(g, g + p + 1, 0.0);
  if (hat)
    if (int rc = grow(dinf[0], inf_cap[0], n_pad, "hipMalloc(diagnostics vector)")) return rc;
  const int grid = rows_grid(INFL_FIRTH);
  if (int rc = grow(dgpart, gpart_cap, (int64_t)(grid + 1) * (p + 1), "hipMalloc(adjusted-score partials)")) return rc;
  if (!firth_is_fused((int)((p + 15) / 16)))
    if (int rc = grow(domega, omega_cap, n_pad, "hipMalloc(score weights)")) return rc;
  InflArgs a{};
  a.hat = hat ? dinf[0] : nullptr;
  a.out = domega;
  a.gpart = dgpart;
  if (int rc = rows_enqueue(INFL_FIRTH, beta, cov, family, link, a)) return rc;
  if (n > 0) {
    double* sum = dgpart + (int64_t)grid * (p + 1);
    HIPCHK(launch_infl_sum(dgpart, grid, (int)p + 1, sum, st));
    HIPCHK(hipMemcpyAsync(g, sum, sizeof(double) * (size_t)(p + 1), hipMemcpyDeviceToHost, st));
    if (hat) HIPCHK(hipMemcpyAsync(hat, dinf[0], sizeof(double) * n, hipMemcpyDeviceToHost, st));
  }
  return rows_sync(&firth_ms);
}

// omega_i = u_i^2 / (1 - h_i)^k of this shard's rows at beta against cov (the global C) into domega, zeros on
// the padding rows: enqueued on the stream (the meat pass stages its zero beta in the same pinned buffer:
// rows_sync(&score_ms) comes first)
int sglm_engine::score_local(const double* beta, const double* cov, int family, int link, int k) {
  InflArgs a{};
  a.hc_k = k;
  return rows_enqueue(INFL_SCORE, beta, k > 0 ? cov : nullptr, family, link, a, true);
}

// out[i] = sqrt(max(0, disp * x_i' cov x_i)) of NEW rows, streamed through predict_new's scratch
int sglm_engine::predict_new_se(const double* X, int64_t nn, int64_t pp, int64_t ldx, const double* cov, double disp,
                                double* out) {
  HIPCHK(hipSetDevice(device));
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nn, ((int64_t)1 << 27) / std::max<int64_t>(pp, 1)));
  if (int rc = ensure_new_rows(pp, chunk)) return rc;
  if (int rc = upload_cov(cov, pp)) return rc;
  const int P = (int)((pp + 15) / 16);
  for (int64_t r0 = 0; r0 < nn; r0 += chunk) {
    const int64_t nr = std::min(chunk, nn - r0);
    if (int rc = h2d_block(dxs, nr, X + r0, ldx, nr, pp)) return rc;
    InflArgs a{};
    a.X = dxs;
    a.ld = nr;
    a.p = (int)pp;
    a.n = nr;
    a.ct = dct;
    a.need_q = 1;
    a.dispersion = disp;
    a.out = dvs;
    HIPCHK(launch_infl(INFL_QFORM, P, a, infl_grid(INFL_QFORM, P, ncu, nr), st));
    HIPCHK(hipMemcpyAsync(out + r0, dvs, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return SGLM_OK;
}

// inv(X'WX) at beta: the pass of sglm_irls_pass (collective over a communicator) and the engine's
// solve rule (Cholesky, or the LU inverse below LU_SWITCH_RATIO; SGLM_ESINGULAR as the fit).
int sglm::vcov_impl(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double* cov) {
  const int64_t p = h->ncols();
  std::vector<double> packed((size_t)packed_len(p));
  if (int rc = h->pass(MODE_IRLS, beta, 0.0, 0.0, opts->family, opts->link, packed.data())) return rc;
  return bread(h, packed.data(), "breeze.linalg.MatrixSingularException: X'WX is singular", cov);
}

int sglm::bread(sglm_engine* h, double* packed, const char* singular, double* C, double* logdet) {
  const int64_t p = h->ncols();
  std::vector<double> x((size_t)p);
  std::unique_ptr<SolverIface> solver = h->make_solver(p);
  const double t0 = now_ms();
  if (const int srv = solver->solve(packed, x.data())) {
    if (srv == SGLM_ESINGULAR) set_error(singular);
    return srv;
  }
  if (int rc = solver->inverse(C)) return rc;
  if (logdet)
    if (int rc = solver->logdet(logdet)) return rc;
  h->solve_ms += now_ms() - t0;
  h->solve_path = solver->path();
  return SGLM_OK;
}

// The row kernel covers resident designs on the fused / narrow paths' range only: anything else is
// refused before any launch.  `what`: the caller's subject and verb ("per-row diagnostics need").
int sglm::require_fused_or_narrow(const sglm_engine* h, const char* what) {
  bool refuse = false;
  for (const sglm_engine* s : h->shards()) refuse = refuse || s->procx.on || s->wide;
  if (!refuse) return SGLM_OK;
  set_error(std::string("requirement failed: ") + what + " a resident design with p <= " +
            std::to_string(16 * MAX_P16) + " columns on the fused / narrow path (procedural shards, wider "
            "designs and SGLM_FORCE_WIDE are not supported)");
  return SGLM_EINVAL;
}

// V = f C M C on the host (p <= 256), one triangle of the second product mirrored
bool sglm::sandwich_product(const std::vector<double>& C, const std::vector<double>& M, int64_t p, double f,
                            double* cov) {
  std::vector<double> T((size_t)(p * p));
  bool finite = true;
  for (double v : M) finite = finite && std::isfinite(v);
  for (int64_t j = 0; j < p && finite; ++j)
    for (int64_t i = 0; i < p; ++i) {
      double s = 0.0;
      for (int64_t l = 0; l < p; ++l) s += C[(size_t)(i + l * p)] * M[(size_t)(l + j * p)];
      T[(size_t)(i + j * p)] = s;
    }
  for (int64_t j = 0; j < p && finite; ++j)
    for (int64_t i = 0; i <= j; ++i) {
      double s = 0.0, t = 0.0;  // (T C)_ij and (T C)_ji: V = (V + V') / 2
      for (int64_t l = 0; l < p; ++l) {
        s += T[(size_t)(i + l * p)] * C[(size_t)(l + j * p)];
        t += T[(size_t)(j + l * p)] * C[(size_t)(l + i * p)];
      }
      const double v = f * (0.5 * (s + t));
      finite = finite && std::isfinite(v);
      cov[i + j * p] = cov[j + i * p] = v;
    }
  return finite;
}

static int influence_shards(sglm_engine* h, const double* beta, const double* cov, const sglm_glm_opts* opts, int rtype,
                            double disp, double* hat, double* resid, double* cooks, double* sum_hat) {
  // shard order: the outputs concatenated in row order, sum h summed in shard order; kernel time: the slowest shard
  const std::vector<sglm_engine*>& shards = h->shards();
  double total = 0.0;
  for (size_t d = 0; d < shards.size(); ++d) {
    const int64_t lo = h->group() ? h->sub_lo[d] : 0;
    double part = 0.0;
    if (int rc = shards[d]->influence_local(beta, cov, opts->family, opts->link, rtype, disp, hat ? hat + lo : nullptr,
                                            resid ? resid + lo : nullptr, cooks ? cooks + lo : nullptr,
                                            sum_hat ? &part : nullptr))
      return rc;
    total += part;
  }
  h->influence_ms = slowest_shard(h, [](const sglm_engine* s) { return s->influence_ms; });
  if (sum_hat) *sum_hat = total;
  return SGLM_OK;
}

// The score weights of every shard (enqueued on all of them, then awaited); kernel time: the slowest shard.
static int score_shards(sglm_engine* h, const double* beta, const double* cov, const sglm_glm_opts* opts, int k) {
  for (sglm_engine* s : h->shards())
    if (int rc = s->score_local(beta, cov, opts->family, opts->link, k)) return rc;
  for (sglm_engine* s : h->shards())
    if (int rc = s->rows_sync(&s->score_ms)) return rc;
  h->score_ms = slowest_shard(h, [](const sglm_engine* s) { return s->score_ms; });
  return SGLM_OK;
}

extern "C" {

int sglm_vcov(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double* cov) {
  if (int rc = check_handle(h)) return rc;
  if (!opts || !beta || !cov || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link, beta, cov");
    return SGLM_EINVAL;
  }
  if (int rc = check_ready(h)) return rc;
  return vcov_impl(h, opts, beta, cov);
}

int sglm_influence(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, int resid_type, double dispersion,
                   double* hat, double* resid, double* cooks, double* sum_hat) {
  if (!opts || !beta || !family_link_valid(opts->family, opts->link) || resid_type < SGLM_RESID_RESPONSE ||
      resid_type > SGLM_RESID_DEVIANCE) {
    set_error("requirement failed: opts with a supported family/link, beta, a residual type of enum sglm_resid_type");
    return SGLM_EINVAL;
  }
  if (!(dispersion > 0.0)) {
    set_error("requirement failed: dispersion > 0");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = require_fused_or_narrow(h, "per-row diagnostics need")) return rc;
  const int64_t p = h->ncols();
  std::vector<double> cov((size_t)(p * p));
  if (int rc = vcov_impl(h, opts, beta, cov.data())) return rc;
  return influence_shards(h, beta, cov.data(), opts, resid_type, dispersion, hat, resid, cooks, sum_hat);
}

int sglm_vcov_robust(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, int hc_type, double* cov,
                     double* meat) {
  if (!opts || !beta || !cov || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link, beta, cov");
    return SGLM_EINVAL;
  }
  if (hc_type < SGLM_HC0 || hc_type > SGLM_HC3) {
    set_error("requirement failed: hc_type one of SGLM_HC0, SGLM_HC1, SGLM_HC2, SGLM_HC3 (enum sglm_hc_type)");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  // as the per-row diagnostics, whose kernel computes the score weights
  if (int rc = require_fused_or_narrow(h, "the sandwich covariance needs")) return rc;
  const int64_t p = h->ncols();
  const int k = hc_type == SGLM_HC2 ? 1 : (hc_type == SGLM_HC3 ? 2 : 0);
  std::vector<double> C((size_t)(p * p)), M((size_t)(p * p)), x((size_t)p);
  if (int rc = vcov_impl(h, opts, beta, C.data())) return rc;
  if (int rc = score_shards(h, beta, C.data(), opts, k)) return rc;
  std::vector<double> packed((size_t)packed_len(p)), zero((size_t)p, 0.0);
  {
    MeatPassScope scope(h);
    if (int rc = h->pass(MODE_IRLS, zero.data(), 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, packed.data())) return rc;
  }
  h->meat_ms = slowest_shard(h, [](const sglm_engine* s) { return s->last_pass_ms; });
  unpack_gram(packed.data(), p, M.data(), x.data());
  double nrows = (double)(h->group() ? h->g_n : h->n);  // HC1: every row of every shard, weight 0 included
  if (hc_type == SGLM_HC1 && !h->group())
    if (int rc = h->allreduce_small(&nrows, 1)) return rc;
  const double f = hc_type == SGLM_HC1 ? nrows / (nrows - (double)p) : 1.0;
  if (!sandwich_product(C, M, p, f, cov)) {
    set_error("requirement failed: the sandwich covariance is not finite (a row with leverage 1 under HC2 / HC3, "
              "or a row whose mean leaves the family's range at beta)");
    return SGLM_EINVAL;
  }
  if (meat) std::memcpy(meat, M.data(), sizeof(double) * M.size());
  return SGLM_OK;
}

int sglm_get_sandwich_ms(sglm_engine* h, double* score_ms, double* meat_ms) {
  if (int rc = check_handle(h)) return rc;
  if (!score_ms || !meat_ms) {
    set_error("requirement failed: score_ms, meat_ms");
    return SGLM_EINVAL;
  }
  *score_ms = h->score_ms;
  *meat_ms = h->meat_ms;
  return SGLM_OK;
}

int sglm_predict_new_se(sglm_engine* h, const double* X, int64_t n, int64_t p, int64_t ldx, const double* cov,
                        double dispersion, double* out) {
  if (int rc = check_handle(h)) return rc;
  if (!X || !cov || !out || n < 0 || p <= 0 || ldx < n || !(dispersion > 0.0)) {
    set_error("requirement failed: X, cov, out, n >= 0, p >= 1, ldx >= n, dispersion > 0");
    return SGLM_EINVAL;
  }
  if (p > 16 * MAX_P16) {
    set_error("requirement failed: se.fit of new rows needs p <= " + std::to_string(16 * MAX_P16) + " columns");
    return SGLM_EINVAL;
  }
  if (n == 0) return SGLM_OK;
  // new rows are scored on the first device
  return h->shards()[0]->predict_new_se(X, n, p, ldx, cov, dispersion, out);
}

int sglm_get_influence_ms(sglm_engine* h, double* kernel_ms) {
  if (int rc = check_handle(h)) return rc;
  if (!kernel_ms) {
    set_error("requirement failed: kernel_ms");
    return SGLM_EINVAL;
  }
  *kernel_ms = h->influence_ms;
  return SGLM_OK;
}

}  // extern "C"
