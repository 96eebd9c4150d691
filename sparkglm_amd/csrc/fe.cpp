// fe.cpp -- one-way fixed-effects GLM fits that absorb the cluster factor (sglm_fit_glm_fe, sglm_fe_pass,
// sglm_vcov_fe; fixest::feglm): the concentrated ("within") IRLS over the segments, the
// combine tree and the cross-shard sum of the cluster-robust covariance (vcov_cluster.cpp), the kernels
// of fe.hip and the Gram pass of the internal engine over the G group rows.
//
// One step at (beta, alpha): o* = offset + alpha_g (fe_offset_kernel); an ordinary pass that reads o* for
// its offset and stores eta; w and the per-segment sums of w z and w (fe_weights_kernel); the segment
// sums of w x (segment_sum_kernel with w where the sandwich passes u); both through the combine tree into
// one buffer S | t | W, summed over shards and ranks in one all-reduce; rows scaled by 1 / sqrt(W_g)
// (fe_scale_kernel) into the internal engine, whose LM Gram pass returns sum s s' / W and sum s t / W; the
// downdate A = X'WX - ..., b = X'Wz - ... on the host.  The fit is glm_drive itself over a Backend whose
// pass is this step: the solve, the stop rule, the trace and the final statistics are sglm_fit_glm's, and
// the fixed effects move by alpha += (t - s' beta+) / W (fe_alpha_kernel) at the start of the next pass,
// when beta+ is known.
//
// What the two-way fits (fe2.cpp) share is here too: the frame of a step entry point (fe_step_mode,
// fe_unpack_step), the bread (fe_bread), the downloads and scans of level buffers, FeScope (engine.hpp).
// The refusals and the finish of a clustered covariance are vcov_cluster.cpp's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "engine.hpp"

using namespace sglm;

// A column whose within-group weighted sum of squares A_jj is below FE_ABSORBED_RATIO (engine.hpp) of X'WX_jj
// is constant within every group (an intercept among them): absorbed by the fixed effects, A is singular.

void sglm_engine::free_fe() {
  dev_free({&dfo, &dalpha, &dfq, &dfqp, &dfg, &dfg2});
  off_override = nullptr;
  fe_stale = true;
  for (hipEvent_t& e : evf) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

// The buffers of a fixed-effects step on this shard (kept until the clusters or the data change)
int sglm_engine::fe_prepare() {
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  if (int rc = ensure_cl_inner()) return rc;
  if (int rc = grow(domega, omega_cap, n_pad, "hipMalloc(working weights)")) return rc;
  for (hipEvent_t& e : evcl)
    if (!e) HIPCHK(hipEventCreate(&e));
  for (hipEvent_t& e : evf)
    if (!e) HIPCHK(hipEventCreate(&e));
  const size_t d = sizeof(double);
  if (!dfo)
    if (int rc = dev_alloc(&dfo, d * (size_t)n_pad, "hipMalloc(effective offset)")) return rc;
  if (!dfq)
    if (int rc = dev_alloc(&dfq, d * (size_t)std::max<int64_t>(2 * cl_nseg, 1), "hipMalloc(segment scalar sums)"))
      return rc;
  if (!dfqp && cl_prow > 0)
    if (int rc = dev_alloc(&dfqp, d * (size_t)(2 * cl_prow), "hipMalloc(scalar combine scratch)")) return rc;
  if (!dalpha) {
    if (int rc = dev_alloc(&dalpha, d * (size_t)cl_G, "hipMalloc(fixed effects)")) return rc;
    HIPCHK(hipMemsetAsync(dalpha, 0, d * (size_t)cl_G, st));
  }
  if (!dfg) {
    if (int rc = dev_alloc(&dfg, d * (size_t)fe_len(), "hipMalloc(group sums)")) return rc;
    fe_stale = true;
  }
  return SGLM_OK;
}

int sglm_engine::set_effects(double* dst, const double* src, int64_t L) {
  HIPCHK(hipSetDevice(device));
  std::vector<double> a((size_t)L, 0.0);
  if (src)
    for (int64_t l = 0; l < L; ++l) a[(size_t)l] = std::isnan(src[l]) ? 0.0 : src[l];
  HIPCHK(hipMemcpyAsync(dst, a.data(), sizeof(double) * a.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return SGLM_OK;
}

// o* = offset + alpha_g into dfo; the passes read it from now on (off_override)
int sglm_engine::fe_offset_local() {
  HIPCHK(hipSetDevice(device));
  FeOffsetArgs a{};
  a.off = doff;
  a.alpha = dalpha;
  a.seg_start = seg_start();
  a.tile_seg = tile_seg();
  a.seg_cluster = seg_cluster();
  a.ntiles = cl_ntiles;
  a.n = n;
  a.ld = n_pad;
  a.out = dfo;
  HIPCHK(launch_fe_offset(a, fe_grid(ncu, cl_ntiles), st));
  off_override = dfo;
  return SGLM_OK;
}

// The row values of `kind` (common.hpp FeKind) and this shard's group sums into dfg: enqueued on the stream
int sglm_engine::fe_sums_local(int kind, int mode, int family, int link, double mu0, double* va, double* vb) {
  HIPCHK(hipSetDevice(device));
  // as S of the cluster-robust covariance: the combine rewrites the rows of the groups that have a segment
  // here and no others, so the buffer is cleared after every cross-shard sum that landed in it
  if (fe_stale) {
    HIPCHK(hipMemsetAsync(dfg, 0, sizeof(double) * (size_t)fe_len(), st));
    fe_stale = false;
  }
  FeArgs a{};
  a.y = dy;
  a.eta = deta;
  a.m = dm;
  a.off = dfo;
  a.prior = dprior;
  a.n = n;
  a.ld = n_pad;
  a.family = family;
  a.link = link;
  a.mode = mode;
  a.kind = kind;
  a.mu0 = mu0;
  a.theta = theta;
  a.seg_start = seg_start();
  a.tile_seg = tile_seg();
  a.ntiles = cl_ntiles;
  a.w = kind == FE_CHECK ? nullptr : domega;
  a.Q = dfq;
  a.va = va;
  a.vb = vb;
  HIPCHK(launch_fe_weights(a, fe_grid(ncu, cl_ntiles), st, evf[0], evf[1]));
  // the sums of w x (u x) as well, then the per-segment scalars: two columns, t | W
  return group_combine_local(kind != FE_CHECK, dfq, dfqp, 2, dfg);
}

// The tail of a step's local sums (fixed effects: dfg; GEE: dgg): with `rows` the segment sums of u x (u: domega)
// through the combine tree into the first p columns of grp, then the ncol per-segment scalars Q through the same
// tree into the columns after them (evcl[2] to evcl[3] spans both trees)
int sglm_engine::group_combine_local(bool rows, const double* Q, double* Qp, int ncol, double* grp) {
  const int64_t ld = cl_inner->n_pad;
  if (rows) {
    ClusterArgs c{};
    c.X = dX;
    c.ld = n_pad;
    c.p = (int)p;
    c.n = n;
    c.u = domega;
    c.seg_start = seg_start();
    c.tile_seg = tile_seg();
    c.ntiles = cl_ntiles;
    c.R = dR;
    HIPCHK(launch_cluster_sum(c, cluster_sum_grid(ncu, n, (int)p), st, evcl[0], evcl[1]));
    if (int rc = combine_clusters(dR, dP, (int)p, grp, ld, evcl[2], nullptr)) return rc;
  }
  return combine_clusters(Q, Qp, ncol, grp + ld * p, ld, nullptr, rows ? evcl[3] : nullptr);
}

int sglm_engine::fe_sync() {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamSynchronize(st));
  return SGLM_OK;
}

// what every entry point requires, before any launch; collective (cluster_count)
int sglm::fe_check(sglm_engine* h, const sglm_glm_opts* opts, int32_t* G, int which) {
  if (!opts || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = require_fused_or_narrow(h, which == SUM_GEE ? "a GEE fit needs" : "a fixed-effects fit needs")) return rc;
  if (int rc = h->theta_check(opts->family)) return rc;
  if (h->group() && h->group_aborted) {
    set_error("the multi-device handle's RCCL group was aborted by an earlier failure; create a new handle");
    return SGLM_ECOMM;
  }
  if (int rc = cluster_count(h, G)) return rc;
  for (sglm_engine* s : h->shards())
    if (int rc = which == SUM_GEE ? s->gee_prepare() : s->fe_prepare()) return rc;
  return SGLM_OK;
}

namespace {

// what the fixed-effects and the GEE steps keep apart: the row kernel's events, the kernel times, the stale mark
struct GroupSide {
  hipEvent_t* ev;
  double* ms;
  bool* stale;
};
GroupSide group_side(sglm_engine* s, int which) {
  return which == SUM_GEE ? GroupSide{s->evg, s->gee_ms, &s->gee_stale} : GroupSide{s->evf, s->fe_ms, &s->fe_stale};
}

// kernel times of the step just synchronised: the slowest shard
int group_times(sglm_engine* h, int which, bool rows) {
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards) {
    const GroupSide g = group_side(s, which);
    HIPCHK(hipSetDevice(s->device));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
    g.ms[0] = ms;
    if (!rows) continue;
    HIPCHK(hipEventElapsedTime(&ms, s->evcl[0], s->evcl[1]));
    g.ms[1] = ms;
    g.ms[2] = 0.0;
    if (!s->cl_levels.empty()) {  // (no level, no combine launch: its events were not recorded)
      HIPCHK(hipEventElapsedTime(&ms, s->evcl[2], s->evcl[3]));
      g.ms[2] = ms;
    }
  }
  double* out = group_side(h, which).ms;
  for (int k = 0; k < 3; ++k)
    for (sglm_engine* s : shards) {
      const double v = group_side(s, which).ms[k];
      out[k] = s == shards[0] ? v : std::max(out[k], v);
    }
  return SGLM_OK;
}

}  // namespace

// After every shard's local sums were enqueued: synchronise, take the kernel times, and sum over shards and ranks
int sglm::group_sums_finish(sglm_engine* h, int which, bool rows) {
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards)
    if (int rc = s->fe_sync()) return rc;
  if (int rc = group_times(h, which, rows)) return rc;
  // the sum over shards or ranks lands in the buffer itself, which this shard's next combine only partly rewrites
  if (h->group() || h->comm.kind != 0)
    for (sglm_engine* s : shards) *group_side(s, which).stale = true;
  return sum_cluster_scores(h, which);
}

// The group sums of `kind` over every shard and rank: shard 0 of every rank ends with bitwise the same dfg
int sglm::fe_group_sums(sglm_engine* h, int kind, int mode, int family, int link, double mu0, double* va, double* vb) {
  for (sglm_engine* s : h->shards())  // (va, vb: one shard's rows -- the two-way fits, which ask for them, have one)
    if (int rc = s->fe_sums_local(kind, mode, family, link, mu0, va, vb)) return rc;
  return group_sums_finish(h, SUM_FE, kind != FE_CHECK);
}

int sglm::absorbed_error(int64_t j) {
  set_error("breeze.linalg.MatrixSingularException: column " + std::to_string(j) + " of X is constant within every "
            "group (an intercept, or a regressor that only varies between groups): the fixed effects absorb it");
  return SGLM_ESINGULAR;
}

int sglm::fe_step_mode(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, int* mode, double* mu0) {
  *mode = MODE_IRLS;
  *mu0 = 0.0;
  if (beta) return SGLM_OK;
  double sums[2];
  if (int rc = h->global_sums(sums)) return rc;
  *mu0 = sums[0] / sums[1];
  *mode = opts->init_mode == SGLM_INIT_MULTIPLE ? MODE_INIT_MULTI : MODE_INIT_SINGLE;
  return SGLM_OK;
}

void sglm::fe_unpack_step(const double* packed, int64_t p, double* A, double* b, double* scalars) {
  std::vector<double> g((size_t)(p * p)), x((size_t)p);
  unpack_gram(packed, p, g.data(), x.data());
  if (A) std::memcpy(A, g.data(), sizeof(double) * g.size());
  if (b) std::memcpy(b, x.data(), sizeof(double) * x.size());
  if (scalars) std::memcpy(scalars, packed + tri_count(p) + p, sizeof(double) * NS);
}

int sglm::fe_bread(sglm_engine* h, double* packed, const char* singular, std::vector<double>& C) {
  const int64_t p = h->ncols();
  std::vector<double> x((size_t)p);
  std::unique_ptr<SolverIface> solver = h->make_solver(p);
  const double t0 = now_ms();
  if (const int srv = solver->solve(packed, x.data())) {
    if (srv == SGLM_ESINGULAR) set_error(singular);
    return srv;
  }
  C.resize((size_t)(p * p));
  if (int rc = solver->inverse(C.data())) return rc;
  h->solve_ms += now_ms() - t0;
  h->solve_path = solver->path();
  return SGLM_OK;
}

int sglm::fe_plain_cov(const std::vector<double>& C, double* cov, double* meat) {
  std::memcpy(cov, C.data(), sizeof(double) * C.size());
  if (meat) std::fill(meat, meat + C.size(), 0.0);
  return SGLM_OK;
}

int sglm::download_cols(sglm_engine* s, const double* buf, int64_t ld, int64_t L, int64_t col0, int64_t ncol,
                        double* out) {
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpy2D(out, sizeof(double) * L, buf + col0 * ld, sizeof(double) * ld, sizeof(double) * L, (size_t)ncol,
                     hipMemcpyDeviceToHost));
  return SGLM_OK;
}

int32_t sglm::count_weighted(const std::vector<double>& W, double* effects) {
  int32_t count = 0;
  for (size_t l = 0; l < W.size(); ++l) {
    if (W[l] > 0.0) count += 1;
    else if (effects) effects[l] = std::numeric_limits<double>::quiet_NaN();
  }
  return count;
}

std::pair<int64_t, int64_t> sglm::uninformative_levels(const std::vector<double>& ab) {
  const size_t L = ab.size() / 2;
  int64_t count = 0, first = -1;
  for (size_t l = 0; l < L; ++l)
    if ((ab[l] == 0.0) != (ab[L + l] == 0.0)) {
      count += 1;
      if (first < 0) first = (int64_t)l;
    }
  return {count, first};
}

namespace {

// alpha += (t - s' beta) / W from the sums of the last step, on shard 0; a group's other shards get a copy
int fe_alpha_step(sglm_engine* h, const double* beta) {
  const std::vector<sglm_engine*>& shards = h->shards();
  sglm_engine* s0 = shards[0];
  HIPCHK(hipSetDevice(s0->device));
  const int64_t p = s0->p;
  std::memcpy(s0->hbeta, beta, sizeof(double) * p);
  HIPCHK(hipMemcpyAsync(s0->dbeta, s0->hbeta, sizeof(double) * p, hipMemcpyHostToDevice, s0->st));
  FeGroupArgs a{};
  a.grp = s0->dfg;
  a.G = s0->cl_G;
  a.ld = s0->cl_inner->n_pad;
  a.p = (int)p;
  a.beta = s0->dbeta;
  a.alpha = s0->dalpha;
  HIPCHK(launch_fe_alpha(a, s0->st));
  if (shards.size() > 1) {
    std::vector<double> al((size_t)s0->cl_G);
    HIPCHK(hipMemcpyAsync(al.data(), s0->dalpha, sizeof(double) * al.size(), hipMemcpyDeviceToHost, s0->st));
    HIPCHK(hipStreamSynchronize(s0->st));
    for (size_t d = 1; d < shards.size(); ++d)
      if (int rc = shards[d]->set_effects(shards[d]->dalpha, al.data(), s0->cl_G)) return rc;
  }
  return SGLM_OK;
}

// The group rows scaled into the internal engine of shard 0 and its LM Gram pass: packed [packed_len(p)]
int fe_group_gram(sglm_engine* h, bool meat, double* packed) {
  sglm_engine* s0 = h->shards()[0];
  sglm_engine* in = s0->cl_inner;
  HIPCHK(hipSetDevice(s0->device));
  FeGroupArgs a{};
  a.grp = s0->dfg;
  a.grp_w = s0->dfg2;
  a.G = s0->cl_G;
  a.ld = in->n_pad;
  a.p = (int)s0->p;
  a.meat = meat ? 1 : 0;
  a.X = in->dX;
  a.y = in->dy;
  HIPCHK(launch_fe_scale(a, s0->st));
  HIPCHK(hipStreamSynchronize(s0->st));  // the internal engine's pass runs on its own stream
  s0->cl_S_stale = true;                 // the cluster-robust covariance's S lives in the same design
  if (int rc = in->pass(MODE_LM_GRAM, nullptr, 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, packed)) return rc;
  h->fe_ms[3] = in->last_pass_ms;
  return SGLM_OK;
}

// One step at the shards' (alpha, o*): packed = lower tri A | b | the pass's scalars, all-reduced
int fe_step(sglm_engine* h, int family, int link, int mode, const double* beta, double mu0, bool check_absorbed,
            double* packed) {
  const int64_t p = h->ncols();
  if (int rc = h->pass(mode, beta, mu0, 0.0, family, link, packed)) return rc;
  if (int rc = fe_group_sums(h, FE_WZ, mode, family, link, mu0)) return rc;
  std::vector<double> down((size_t)packed_len(p));
  if (int rc = fe_group_gram(h, false, down.data())) return rc;
  for (int64_t j = 0; j < p; ++j) {
    const int64_t jj = j * (j + 1) / 2 + j;
    if (check_absorbed && packed[jj] > 0.0 && !(packed[jj] - down[(size_t)jj] > FE_ABSORBED_RATIO * packed[jj]))
      return absorbed_error(j);
  }
  for (int64_t k = 0; k < tri_count(p) + p; ++k) packed[k] -= down[(size_t)k];
  return SGLM_OK;
}

int fe_offsets(sglm_engine* h) {
  for (sglm_engine* s : h->shards())
    if (int rc = s->fe_offset_local()) return rc;
  return SGLM_OK;
}

int fe_set_alpha_all(sglm_engine* h, const double* alpha) {
  for (sglm_engine* s : h->shards())
    if (int rc = s->set_effects(s->dalpha, alpha, s->cl_G)) return rc;
  return SGLM_OK;
}

// columns [col0, col0 + ncol) of shard 0's group sums, the first G rows of each, to the host
int fe_download(sglm_engine* h, int64_t col0, int64_t ncol, double* out) {
  sglm_engine* s0 = h->shards()[0];
  return download_cols(s0, s0->dfg, s0->cl_inner->n_pad, s0->cl_G, col0, ncol, out);
}

// The fit's Backend: glm_drive's pass is the fixed-effects step; no deviance-only passes (every pass's sums
// move alpha), no in-pass statistics (the passes store eta for the weights kernel).
struct FeBackend : public Backend {
  sglm_engine* h;
  explicit FeBackend(sglm_engine* handle) : h(handle) {}
  int64_t ncols() const override { return h->ncols(); }
  int npart() const override { return h->npart(); }
  int global_sums(double* out2) override { return h->global_sums(out2); }
  int pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override {
    (void)ybar;
    if (beta)
      if (int rc = fe_alpha_step(h, beta)) return rc;
    if (int rc = fe_offsets(h)) return rc;
    return fe_step(h, family, link, mode, beta, mu0, true, packed);
  }
  int stats(int mode, const double* beta, double mu0, double ybar, int family, int link, double* s) override {
    return h->stats(mode, beta, mu0, ybar, family, link, s);
  }
  std::unique_ptr<SolverIface> make_solver(int64_t p) override { return h->make_solver(p); }
};

// Groups without a finite alpha: the rows of positive prior weight all have y = 0 (or all y = m)
int fe_uninformative(sglm_engine* h, int family, int link, int32_t G) {
  if (family != FAM_BINOMIAL && family != FAM_POISSON && family != FAM_NEGBIN) return SGLM_OK;
  if (int rc = fe_group_sums(h, FE_CHECK, MODE_IRLS, family, link, 0.0)) return rc;
  std::vector<double> ab((size_t)(2 * G));
  if (int rc = fe_download(h, h->ncols(), 2, ab.data())) return rc;
  const auto [count, first] = uninformative_levels(ab);
  if (count == 0) return SGLM_OK;
  set_error("requirement failed: " + std::to_string(count) + " group(s) have no finite fixed effect -- every row of "
            "positive prior weight has y = 0" + (family == FAM_BINOMIAL ? " or y = m" : "") + "; the first is group " +
            std::to_string(first) + " (drop their rows, as fixest does)");
  return SGLM_EINVAL;
}

}  // namespace

extern "C" {

int sglm_fit_glm_fe(sglm_engine* h, const sglm_glm_opts* opts, sglm_preglm* out, double* alpha, sglm_fe_info* info) {
  if (!out || !out->coefs || !out->std_err || !alpha) {
    set_error("requirement failed: out, out->coefs, out->std_err, alpha");
    return SGLM_EINVAL;
  }
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G)) return rc;
  FeScope scope(h);
  if (int rc = fe_set_alpha_all(h, nullptr)) return rc;
  if (int rc = fe_uninformative(h, opts->family, opts->link, G)) return rc;
  FeBackend be(h);
  if (int rc = glm_drive(be, *opts, out)) return rc;
  h->solve_ms += be.solve_ms;
  h->solve_path = be.solve_path;
  // alpha of the last pass (at out->coefs) and the W of that pass: a group without weight has no alpha
  std::vector<double> W((size_t)G);
  sglm_engine* s0 = h->shards()[0];
  HIPCHK(hipSetDevice(s0->device));
  HIPCHK(hipMemcpy(alpha, s0->dalpha, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost));
  if (int rc = fe_download(h, h->ncols() + 1, 1, W.data())) return rc;
  const int32_t geff = count_weighted(W, alpha);
  if (info) {
    info->G_eff = geff;
    info->df_residual = out->nrow - (double)h->ncols() - (double)geff;
    info->weights_ms = h->fe_ms[0];
    info->sum_ms = h->fe_ms[1];
    info->combine_ms = h->fe_ms[2];
    info->gram_ms = h->fe_ms[3];
  }
  return SGLM_OK;
}

int sglm_fe_pass(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, const double* alpha, double* A,
                 double* b, double* group, double* scalars) {
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G)) return rc;
  FeScope scope(h);
  const int64_t p = h->ncols();
  double mu0;
  int mode;
  if (int rc = fe_step_mode(h, opts, beta, &mode, &mu0)) return rc;
  if (int rc = fe_set_alpha_all(h, alpha)) return rc;
  if (int rc = fe_offsets(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p));
  if (int rc = fe_step(h, opts->family, opts->link, mode, beta, mu0, false, packed.data())) return rc;
  fe_unpack_step(packed.data(), p, A, b, scalars);
  if (group)
    if (int rc = fe_download(h, 0, p + 2, group)) return rc;
  return SGLM_OK;
}

int sglm_vcov_fe(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, const double* alpha, int cluster,
                 int hc_type, int cadjust, double* cov, double* meat) {
  if (!beta || !alpha || !cov) {
    set_error("requirement failed: beta, alpha, cov");
    return SGLM_EINVAL;
  }
  if (cluster)
    if (int rc = check_cluster_hc(hc_type)) return rc;
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G)) return rc;
  if (cluster)
    if (int rc = check_cadjust(cadjust, G)) return rc;
  FeScope scope(h);
  const int64_t p = h->ncols();
  sglm_engine* s0 = h->shards()[0];
  if (int rc = fe_set_alpha_all(h, alpha)) return rc;
  if (int rc = fe_offsets(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p)), C, M((size_t)(p * p)), x((size_t)p);
  if (int rc = fe_step(h, opts->family, opts->link, MODE_IRLS, beta, 0.0, true, packed.data())) return rc;
  const char* singular = "breeze.linalg.MatrixSingularException: the within-group X'WX is singular";
  if (int rc = fe_bread(h, packed.data(), singular, C)) return rc;
  if (!cluster) return fe_plain_cov(C, cov, meat);
  // the w-weighted sums s | W stay in dfg2 while the u-weighted ones S | U are formed in dfg
  HIPCHK(hipSetDevice(s0->device));
  if (!s0->dfg2)
    if (int rc = sglm_engine::dev_alloc(&s0->dfg2, sizeof(double) * (size_t)s0->fe_len(), "hipMalloc(group sums)"))
      return rc;
  HIPCHK(hipMemcpyAsync(s0->dfg2, s0->dfg, sizeof(double) * (size_t)s0->fe_len(), hipMemcpyDeviceToDevice, s0->st));
  std::vector<double> W((size_t)G);
  if (int rc = fe_download(h, p + 1, 1, W.data())) return rc;
  const int32_t geff = count_weighted(W, nullptr);
  if (int rc = fe_group_sums(h, FE_SCORE, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  if (int rc = fe_group_gram(h, true, packed.data())) return rc;
  unpack_gram(packed.data(), p, M.data(), x.data());
  double nrows = (double)(h->group() ? h->g_n : h->n);  // every row of every shard, weight 0 included
  if (hc_type == SGLM_HC1 && !h->group())
    if (int rc = h->allreduce_small(&nrows, 1)) return rc;
  return clustered_finish(hc_type, nrows, p, geff, G, cadjust, C, M, "(beta, alpha)", cov, meat);
}

int sglm_get_fe_ms(sglm_engine* h, double* weights_ms, double* sum_ms, double* combine_ms, double* gram_ms) {
  if (int rc = check_handle(h)) return rc;
  if (!weights_ms || !sum_ms || !combine_ms || !gram_ms) {
    set_error("requirement failed: weights_ms, sum_ms, combine_ms, gram_ms");
    return SGLM_EINVAL;
  }
  *weights_ms = h->fe_ms[0];
  *sum_ms = h->fe_ms[1];
  *combine_ms = h->fe_ms[2];
  *gram_ms = h->fe_ms[3];
  return SGLM_OK;
}

}  // extern "C"
