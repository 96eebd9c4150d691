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
// What the two-way fits (fe2.cpp) and the GEE fits (gee.cpp) share is here too.  The host frame of a step over
// the cluster factor, written once over the sglm_engine::GroupSums it works on (fe or gee): group_prepare /
// free_group, group_sums_local (stale clear, row kernel, both combine trees), group_sums_finish (times, the sum
// over shards and ranks), group_gram (scale launch, the internal engine's Gram pass), keep_group_sums, and
// drive_step_fit over a StepBackend.  The frame of a step entry point (fe_check, fe_step_mode,
// fe_unpack_step), the downloads and scans of level buffers, FeScope (engine.hpp).
// The refusals and the finish of a clustered covariance are vcov_cluster.cpp's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "engine.hpp"

using namespace sglm;

// A column whose within-group weighted sum of squares A_jj is below FE_ABSORBED_RATIO (engine.hpp) of X'WX_jj
// is constant within every group (an intercept among them): absorbed by the fixed effects, A is singular.

void sglm_engine::free_group(GroupSums& gs) {
  dev_free({&gs.q, &gs.qp, &gs.g, &gs.g2});
  gs.stale = true;
  for (hipEvent_t& e : gs.ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

void sglm_engine::free_fe() {
  dev_free({&dfo, &dalpha});
  off_override = nullptr;
  free_group(fe);
}

int sglm_engine::group_prepare(GroupSums& gs) {
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  if (int rc = ensure_cl_inner()) return rc;
  if (int rc = grow(domega, omega_cap, n_pad, "hipMalloc(working weights)")) return rc;
  for (hipEvent_t& e : evcl)
    if (!e) HIPCHK(hipEventCreate(&e));
  for (hipEvent_t& e : gs.ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  const size_t d = sizeof(double);
  if (!gs.q)
    if (int rc = dev_alloc(&gs.q, d * (size_t)std::max<int64_t>(gs.nq * cl_nseg, 1), "hipMalloc(segment scalar sums)"))
      return rc;
  if (!gs.qp && cl_prow > 0)
    if (int rc = dev_alloc(&gs.qp, d * (size_t)(gs.nq * cl_prow), "hipMalloc(scalar combine scratch)")) return rc;
  if (!gs.g) {
    if (int rc = dev_alloc(&gs.g, d * (size_t)group_len(gs), "hipMalloc(group sums)")) return rc;
    gs.stale = true;
  }
  return SGLM_OK;
}

// The buffers of a fixed-effects step on this shard
int sglm_engine::fe_prepare() {
  if (int rc = group_prepare(fe)) return rc;
  const size_t d = sizeof(double);
  if (!dfo)
    if (int rc = dev_alloc(&dfo, d * (size_t)n_pad, "hipMalloc(effective offset)")) return rc;
  if (!dalpha) {
    if (int rc = dev_alloc(&dalpha, d * (size_t)cl_G, "hipMalloc(fixed effects)")) return rc;
    HIPCHK(hipMemsetAsync(dalpha, 0, d * (size_t)cl_G, st));
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

int sglm_engine::group_sums_local(GroupSums& gs, RowLaunch launch, bool rows, int kind, int mode, int family, int link,
                                  double mu0, const double* off, double* va, double* vb) {
  HIPCHK(hipSetDevice(device));
  // as S of the cluster-robust covariance: the combine rewrites the rows of the groups that have a segment
  // here and no others, so the buffer is cleared after every cross-shard sum that landed in it
  if (gs.stale) {
    HIPCHK(hipMemsetAsync(gs.g, 0, sizeof(double) * (size_t)group_len(gs), st));
    gs.stale = false;
  }
  SegRowArgs a{};
  a.y = dy;
  a.eta = deta;
  a.m = dm;
  a.off = off;
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
  a.w = rows ? domega : nullptr;
  a.Q = gs.q;
  a.va = va;
  a.vb = vb;
  HIPCHK(launch(a, fe_grid(ncu, cl_ntiles), st, gs.ev[0], gs.ev[1]));
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
    if (int rc = combine_clusters(dR, dP, (int)p, gs.g, ld, evcl[2], nullptr)) return rc;
  }
  return combine_clusters(gs.q, gs.qp, gs.nq, gs.g + ld * p, ld, nullptr, rows ? evcl[3] : nullptr);
}

// The row values of `kind` (common.hpp FeKind: w or u into domega; at the effective offset) and the sums of w x
// (u x), t | W into fe.g
int sglm_engine::fe_sums_local(int kind, int mode, int family, int link, double mu0, double* va, double* vb) {
  return group_sums_local(fe, launch_fe_weights, kind != FE_CHECK, kind, mode, family, link, mu0, dfo, va, vb);
}

int sglm_engine::keep_group_sums(GroupSums& gs) {
  HIPCHK(hipSetDevice(device));
  const size_t bytes = sizeof(double) * (size_t)group_len(gs);
  if (!gs.g2)
    if (int rc = dev_alloc(&gs.g2, bytes, "hipMalloc(group sums)")) return rc;
  HIPCHK(hipMemcpyAsync(gs.g2, gs.g, bytes, hipMemcpyDeviceToDevice, st));
  return SGLM_OK;
}

int sglm_engine::fe_sync() {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamSynchronize(st));
  return SGLM_OK;
}

// what every entry point requires, before any launch; collective (cluster_count)
int sglm::fe_check(sglm_engine* h, const sglm_glm_opts* opts, int32_t* G, const char* needs,
                   int (sglm_engine::*prepare)()) {
  if (!opts || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = require_fused_or_narrow(h, needs)) return rc;
  if (int rc = h->theta_check(opts->family)) return rc;
  if (h->group() && h->group_aborted) {
    set_error("the multi-device handle's RCCL group was aborted by an earlier failure; create a new handle");
    return SGLM_ECOMM;
  }
  if (int rc = cluster_count(h, G)) return rc;
  for (sglm_engine* s : h->shards())
    if (int rc = (s->*prepare)()) return rc;
  return SGLM_OK;
}

namespace {

// kernel times of the step just synchronised: the slowest shard
int group_times(sglm_engine* h, GroupSumsOf gs, bool rows) {
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards) {
    double* sms = (s->*gs).ms;
    HIPCHK(hipSetDevice(s->device));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, (s->*gs).ev[0], (s->*gs).ev[1]));
    sms[0] = ms;
    if (!rows) continue;
    HIPCHK(hipEventElapsedTime(&ms, s->evcl[0], s->evcl[1]));
    sms[1] = ms;
    sms[2] = 0.0;
    if (!s->cl_levels.empty()) {  // (no level, no combine launch: its events were not recorded)
      HIPCHK(hipEventElapsedTime(&ms, s->evcl[2], s->evcl[3]));
      sms[2] = ms;
    }
  }
  for (int k = 0; k < 3; ++k) (h->*gs).ms[k] = slowest_shard(h, [&](const sglm_engine* s) { return (s->*gs).ms[k]; });
  return SGLM_OK;
}

}  // namespace

int sglm::group_sums_finish(sglm_engine* h, GroupSumsOf gs, bool rows) {
  const std::vector<sglm_engine*>& shards = h->shards();
  for (sglm_engine* s : shards)
    if (int rc = s->fe_sync()) return rc;
  if (int rc = group_times(h, gs, rows)) return rc;
  // the sum over shards or ranks lands in the buffer itself, which this shard's next combine only partly rewrites
  if (h->group() || h->comm.kind != 0)
    for (sglm_engine* s : shards) (s->*gs).stale = true;
  return sum_cluster_scores(h, [gs](sglm_engine* s) { return (s->*gs).g; }, shards[0]->group_len(shards[0]->*gs));
}

int sglm::group_gram(sglm_engine* h, GroupSumsOf gs, hipError_t (*scale)(const GroupArgs&, hipStream_t), bool meat,
                     double rho, double* packed) {
  sglm_engine* s0 = h->shards()[0];
  sglm_engine* in = s0->cl_inner;
  HIPCHK(hipSetDevice(s0->device));
  GroupArgs a{};
  a.grp = (s0->*gs).g;
  a.grp2 = meat ? (s0->*gs).g2 : (s0->*gs).g;
  a.G = s0->cl_G;
  a.ld = in->n_pad;
  a.p = (int)s0->p;
  a.meat = meat ? 1 : 0;
  a.rho = rho;
  a.X = in->dX;
  a.y = in->dy;
  HIPCHK(scale(a, s0->st));
  HIPCHK(hipStreamSynchronize(s0->st));  // the internal engine's pass runs on its own stream
  s0->cl_S_stale = true;                 // the cluster-robust covariance's S lives in the same design
  if (int rc = in->pass(MODE_LM_GRAM, nullptr, 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, packed)) return rc;
  (h->*gs).ms[3] = in->last_pass_ms;
  return SGLM_OK;
}

int sglm::drive_step_fit(StepBackend& be, const sglm_glm_opts& opts, sglm_preglm* out) {
  if (int rc = glm_drive(be, opts, out)) return rc;
  be.h->solve_ms += be.solve_ms;
  be.h->solve_path = be.solve_path;
  return SGLM_OK;
}

// The group sums of `kind` over every shard and rank: shard 0 of every rank ends with bitwise the same fe.g
int sglm::fe_group_sums(sglm_engine* h, int kind, int mode, int family, int link, double mu0, double* va, double* vb) {
  for (sglm_engine* s : h->shards())  // (va, vb: one shard's rows -- the two-way fits, which ask for them, have one)
    if (int rc = s->fe_sums_local(kind, mode, family, link, mu0, va, vb)) return rc;
  return group_sums_finish(h, &sglm_engine::fe, kind != FE_CHECK);
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
  GroupArgs a{};
  a.grp = s0->fe.g;
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

// One step at the shards' (alpha, o*): packed = lower tri A | b | the pass's scalars, all-reduced
int fe_step(sglm_engine* h, int family, int link, int mode, const double* beta, double mu0, bool check_absorbed,
            double* packed) {
  const int64_t p = h->ncols();
  if (int rc = h->pass(mode, beta, mu0, 0.0, family, link, packed)) return rc;
  if (int rc = fe_group_sums(h, FE_WZ, mode, family, link, mu0)) return rc;
  std::vector<double> down((size_t)packed_len(p));
  if (int rc = group_gram(h, &sglm_engine::fe, launch_fe_scale, false, 0.0, down.data())) return rc;
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
  return download_cols(s0, s0->fe.g, s0->cl_inner->n_pad, s0->cl_G, col0, ncol, out);
}

// The fit's Backend: glm_drive's pass is the fixed-effects step; no deviance-only passes (every pass's sums
// move alpha), no in-pass statistics (the passes store eta for the weights kernel).
struct FeBackend : public StepBackend {
  using StepBackend::StepBackend;
  int pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override {
    (void)ybar;
    if (beta)
      if (int rc = fe_alpha_step(h, beta)) return rc;
    if (int rc = fe_offsets(h)) return rc;
    return fe_step(h, family, link, mode, beta, mu0, true, packed);
  }
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
  if (int rc = drive_step_fit(be, *opts, out)) return rc;
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
    info->weights_ms = h->fe.ms[0];
    info->sum_ms = h->fe.ms[1];
    info->combine_ms = h->fe.ms[2];
    info->gram_ms = h->fe.ms[3];
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
  if (int rc = fe_set_alpha_all(h, alpha)) return rc;
  if (int rc = fe_offsets(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p)), C((size_t)(p * p)), M((size_t)(p * p)), x((size_t)p);
  if (int rc = fe_step(h, opts->family, opts->link, MODE_IRLS, beta, 0.0, true, packed.data())) return rc;
  const char* singular = "breeze.linalg.MatrixSingularException: the within-group X'WX is singular";
  if (int rc = bread(h, packed.data(), singular, C.data())) return rc;
  if (!cluster) return fe_plain_cov(C, cov, meat);
  // the w-weighted sums s | W stay in g2 while the u-weighted ones S | U are formed in g
  if (int rc = h->shards()[0]->keep_group_sums(h->shards()[0]->fe)) return rc;
  std::vector<double> W((size_t)G);
  if (int rc = fe_download(h, p + 1, 1, W.data())) return rc;
  const int32_t geff = count_weighted(W, nullptr);
  if (int rc = fe_group_sums(h, FE_SCORE, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  if (int rc = group_gram(h, &sglm_engine::fe, launch_fe_scale, true, 0.0, packed.data())) return rc;
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
  *weights_ms = h->fe.ms[0];
  *sum_ms = h->fe.ms[1];
  *combine_ms = h->fe.ms[2];
  *gram_ms = h->fe.ms[3];
  return SGLM_OK;
}

}  // extern "C"
