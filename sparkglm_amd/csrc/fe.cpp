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

// alpha [G] to the device; a NaN (a group without weight) is read as 0; null: zeros
int sglm_engine::fe_set_alpha(const double* alpha) {
  HIPCHK(hipSetDevice(device));
  std::vector<double> a((size_t)cl_G, 0.0);
  if (alpha)
    for (int32_t g = 0; g < cl_G; ++g) a[(size_t)g] = std::isnan(alpha[g]) ? 0.0 : alpha[g];
  HIPCHK(hipMemcpyAsync(dalpha, a.data(), sizeof(double) * a.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return SGLM_OK;
}

// o* = offset + alpha_g into dfo; the passes read it from now on (off_override)
int sglm_engine::fe_offset_local() {
  HIPCHK(hipSetDevice(device));
  FeOffsetArgs a{};
  a.off = doff;
  a.alpha = dalpha;
  a.seg_start = dclidx;
  a.tile_seg = dclidx + cl_nseg + 2;
  a.seg_cluster = dclidx + cl_segcl_off;
  a.ntiles = cl_ntiles;
  a.n = n;
  a.ld = n_pad;
  a.out = dfo;
  HIPCHK(launch_fe_offset(a, fe_grid(ncu, cl_ntiles), st));
  off_override = dfo;
  return SGLM_OK;
}

// The row values of `kind` (common.hpp FeKind) and this shard's group sums into dfg: enqueued on the stream
int sglm_engine::fe_sums_local(int kind, int mode, int family, int link, double mu0) {
  HIPCHK(hipSetDevice(device));
  const int64_t ld = cl_inner->n_pad;
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
  a.seg_start = dclidx;
  a.tile_seg = dclidx + cl_nseg + 2;
  a.ntiles = cl_ntiles;
  a.w = kind == FE_CHECK ? nullptr : domega;
  a.Q = dfq;
  HIPCHK(launch_fe_weights(a, fe_grid(ncu, cl_ntiles), st, evf[0], evf[1]));
  const bool rows = kind != FE_CHECK;  // the sums of w x (u x) as well
  if (rows) {
    ClusterArgs c{};
    c.X = dX;
    c.ld = n_pad;
    c.p = (int)p;
    c.n = n;
    c.u = domega;
    c.seg_start = a.seg_start;
    c.tile_seg = a.tile_seg;
    c.ntiles = cl_ntiles;
    c.R = dR;
    HIPCHK(launch_cluster_sum(c, cluster_sum_grid(ncu, n, (int)p), st, evcl[0], evcl[1]));
  }
  const int64_t* cl_seg = a.tile_seg + cl_ntiles + 1;
  for (size_t l = 0; l < cl_levels.size(); ++l) {
    const CombineLevel& lv = cl_levels[l];
    CombineArgs c{};
    c.idx = l == 0 ? cl_seg : nullptr;
    c.chunk_start = dclidx + lv.start_off;
    c.chunk_dst = dclidx + lv.dst_off;
    c.nchunk = lv.nchunk;
    c.ldS = ld;
    if (rows) {
      c.in = l == 0 ? dR : dP + lv.in_row * p;
      c.p = (int)p;
      c.S = dfg;
      c.out = dP ? dP + lv.out_row * p : nullptr;
      HIPCHK(launch_cluster_combine(c, ncu, st, l == 0 ? evcl[2] : nullptr, nullptr));
    }
    // the per-segment scalars through the same tree: two columns, t | W
    c.in = l == 0 ? dfq : dfqp + lv.in_row * 2;
    c.p = 2;
    c.S = dfg + ld * p;
    c.out = dfqp ? dfqp + lv.out_row * 2 : nullptr;
    HIPCHK(launch_cluster_combine(c, ncu, st, nullptr, rows && l + 1 == cl_levels.size() ? evcl[3] : nullptr));
  }
  return SGLM_OK;
}

int sglm_engine::fe_sync() {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamSynchronize(st));
  return SGLM_OK;
}

namespace {

// While it lives every IRLS pass of the handle's shards stores eta; at its end the passes read the shards'
// own offsets again.
struct FeScope {
  sglm_engine* h;
  explicit FeScope(sglm_engine* handle) : h(handle) {
    for (sglm_engine* s : h->shards()) s->want_eta = true;
  }
  ~FeScope() {
    for (sglm_engine* s : h->shards()) {
      s->want_eta = false;
      s->off_override = nullptr;
    }
  }
};

}  // namespace

// what every entry point requires, before any launch; collective (cluster_count)
int sglm::fe_check(sglm_engine* h, const sglm_glm_opts* opts, int32_t* G) {
  if (!opts || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = require_fused_or_narrow(h, "a fixed-effects fit needs")) return rc;
  if (int rc = h->theta_check(opts->family)) return rc;
  if (h->group() && h->group_aborted) {
    set_error("the multi-device handle's RCCL group was aborted by an earlier failure; create a new handle");
    return SGLM_ECOMM;
  }
  if (int rc = cluster_count(h, G)) return rc;
  for (sglm_engine* s : h->shards())
    if (int rc = s->fe_prepare()) return rc;
  return SGLM_OK;
}

namespace {

// kernel times of the step just synchronised: the slowest shard
int fe_times(sglm_engine* h, bool rows) {
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards) {
    HIPCHK(hipSetDevice(s->device));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s->evf[0], s->evf[1]));
    s->fe_ms[0] = ms;
    if (!rows) continue;
    HIPCHK(hipEventElapsedTime(&ms, s->evcl[0], s->evcl[1]));
    s->fe_ms[1] = ms;
    s->fe_ms[2] = 0.0;
    if (!s->cl_levels.empty()) {  // (no level, no combine launch: its events were not recorded)
      HIPCHK(hipEventElapsedTime(&ms, s->evcl[2], s->evcl[3]));
      s->fe_ms[2] = ms;
    }
  }
  for (int k = 0; k < 3; ++k)
    for (const sglm_engine* s : shards) h->fe_ms[k] = s == shards[0] ? s->fe_ms[k] : std::max(h->fe_ms[k], s->fe_ms[k]);
  return SGLM_OK;
}

}  // namespace

// The group sums of `kind` over every shard and rank: shard 0 of every rank ends with bitwise the same dfg
int sglm::fe_group_sums(sglm_engine* h, int kind, int mode, int family, int link, double mu0) {
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards)
    if (int rc = s->fe_sums_local(kind, mode, family, link, mu0)) return rc;
  for (sglm_engine* s : shards)
    if (int rc = s->fe_sync()) return rc;
  if (int rc = fe_times(h, kind != FE_CHECK)) return rc;
  // the sum over shards or ranks lands in dfg itself, which this shard's next combine only partly rewrites
  if (h->group() || h->comm.kind != 0)
    for (sglm_engine* s : shards) s->fe_stale = true;
  return sum_cluster_scores(h, true);
}

int sglm::absorbed_error(int64_t j) {
  set_error("breeze.linalg.MatrixSingularException: column " + std::to_string(j) + " of X is constant within every "
            "group (an intercept, or a regressor that only varies between groups): the fixed effects absorb it");
  return SGLM_ESINGULAR;
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
      if (int rc = shards[d]->fe_set_alpha(al.data())) return rc;
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
    if (int rc = s->fe_set_alpha(alpha)) return rc;
  return SGLM_OK;
}

// columns [col0, col0 + ncol) of shard 0's group sums, the first G rows of each, to the host
int fe_download(sglm_engine* h, const double* buf, int64_t col0, int64_t ncol, double* out) {
  sglm_engine* s0 = h->shards()[0];
  HIPCHK(hipSetDevice(s0->device));
  const int64_t ld = s0->cl_inner->n_pad, G = s0->cl_G;
  HIPCHK(hipMemcpy2D(out, sizeof(double) * G, buf + col0 * ld, sizeof(double) * ld, sizeof(double) * G, (size_t)ncol,
                     hipMemcpyDeviceToHost));
  return SGLM_OK;
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
  if (int rc = fe_download(h, h->shards()[0]->dfg, h->ncols(), 2, ab.data())) return rc;
  int64_t count = 0, first = -1;
  for (int32_t g = 0; g < G; ++g)
    if ((ab[(size_t)g] == 0.0) != (ab[(size_t)(G + g)] == 0.0)) {  // both 0: no row of positive weight
      count += 1;
      if (first < 0) first = g;
    }
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
  if (int rc = fe_download(h, s0->dfg, h->ncols() + 1, 1, W.data())) return rc;
  int32_t geff = 0;
  for (int32_t g = 0; g < G; ++g) {
    if (W[(size_t)g] > 0.0) geff += 1;
    else alpha[g] = std::numeric_limits<double>::quiet_NaN();
  }
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
  double mu0 = 0.0;
  int mode = MODE_IRLS;
  if (!beta) {
    double sums[2];
    if (int rc = h->global_sums(sums)) return rc;
    mu0 = sums[0] / sums[1];
    mode = opts->init_mode == SGLM_INIT_MULTIPLE ? MODE_INIT_MULTI : MODE_INIT_SINGLE;
  }
  if (int rc = fe_set_alpha_all(h, alpha)) return rc;
  if (int rc = fe_offsets(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p)), g((size_t)(p * p)), x((size_t)p);
  if (int rc = fe_step(h, opts->family, opts->link, mode, beta, mu0, false, packed.data())) return rc;
  unpack_gram(packed.data(), p, g.data(), x.data());
  if (A) std::memcpy(A, g.data(), sizeof(double) * g.size());
  if (b) std::memcpy(b, x.data(), sizeof(double) * x.size());
  if (scalars) std::memcpy(scalars, packed.data() + tri_count(p) + p, sizeof(double) * NS);
  if (group)
    if (int rc = fe_download(h, h->shards()[0]->dfg, 0, p + 2, group)) return rc;
  return SGLM_OK;
}

int sglm_vcov_fe(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, const double* alpha, int cluster,
                 int hc_type, int cadjust, double* cov, double* meat) {
  if (!beta || !alpha || !cov) {
    set_error("requirement failed: beta, alpha, cov");
    return SGLM_EINVAL;
  }
  if (cluster && hc_type != SGLM_HC0 && hc_type != SGLM_HC1) {
    set_error("requirement failed: hc_type SGLM_HC0 or SGLM_HC1 under clustering (HC2 / HC3 need per-cluster "
              "leverage blocks, which the engine does not form)");
    return SGLM_EINVAL;
  }
  int32_t G = 0;
  if (int rc = fe_check(h, opts, &G)) return rc;
  if (cluster && cadjust && G < 2) {
    set_error("requirement failed: cadjust (the factor G / (G - 1)) needs G >= 2 clusters");
    return SGLM_EINVAL;
  }
  FeScope scope(h);
  const int64_t p = h->ncols();
  const std::vector<sglm_engine*>& shards = h->shards();
  sglm_engine* s0 = shards[0];
  if (int rc = fe_set_alpha_all(h, alpha)) return rc;
  if (int rc = fe_offsets(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p)), C((size_t)(p * p)), M((size_t)(p * p)), x((size_t)p);
  if (int rc = fe_step(h, opts->family, opts->link, MODE_IRLS, beta, 0.0, true, packed.data())) return rc;
  std::unique_ptr<SolverIface> solver = h->make_solver(p);
  const double t0 = now_ms();
  if (const int srv = solver->solve(packed.data(), x.data())) {
    if (srv == SGLM_ESINGULAR) set_error("breeze.linalg.MatrixSingularException: the within-group X'WX is singular");
    return srv;
  }
  if (int rc = solver->inverse(C.data())) return rc;
  h->solve_ms += now_ms() - t0;
  h->solve_path = solver->path();
  if (!cluster) {
    std::memcpy(cov, C.data(), sizeof(double) * C.size());
    if (meat) std::fill(meat, meat + p * p, 0.0);
    return SGLM_OK;
  }
  // the w-weighted sums s | W stay in dfg2 while the u-weighted ones S | U are formed in dfg
  HIPCHK(hipSetDevice(s0->device));
  if (!s0->dfg2)
    if (int rc = sglm_engine::dev_alloc(&s0->dfg2, sizeof(double) * (size_t)s0->fe_len(), "hipMalloc(group sums)"))
      return rc;
  HIPCHK(hipMemcpyAsync(s0->dfg2, s0->dfg, sizeof(double) * (size_t)s0->fe_len(), hipMemcpyDeviceToDevice, s0->st));
  std::vector<double> W((size_t)G);
  if (int rc = fe_download(h, s0->dfg, p + 1, 1, W.data())) return rc;
  int32_t geff = 0;
  for (double w : W) geff += w > 0.0 ? 1 : 0;
  if (int rc = fe_group_sums(h, FE_SCORE, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  if (int rc = fe_group_gram(h, true, packed.data())) return rc;
  unpack_gram(packed.data(), p, M.data(), x.data());
  double nrows = (double)(h->group() ? h->g_n : h->n);  // every row of every shard, weight 0 included
  if (hc_type == SGLM_HC1 && !h->group())
    if (int rc = h->allreduce_small(&nrows, 1)) return rc;
  double f = hc_type == SGLM_HC1 ? (nrows - 1.0) / (nrows - (double)p - (double)geff) : 1.0;
  if (cadjust) f *= (double)G / ((double)G - 1.0);
  if (!sandwich_product(C, M, p, f, cov)) {
    set_error("requirement failed: the cluster-robust covariance is not finite (a row whose mean leaves the "
              "family's range at (beta, alpha))");
    return SGLM_EINVAL;
  }
  if (meat) std::memcpy(meat, M.data(), sizeof(double) * M.size());
  return SGLM_OK;
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
