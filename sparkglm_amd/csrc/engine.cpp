// engine.cpp -- the C ABI (include/sglm.h) over the HIP backend: the engine's core.
//
// One sglm_engine (engine.hpp) drives one HIP device: it owns the row shard resident in HBM (X
// column-major with a leading dimension padded to the 32-row block, y / m / offset /
// prior, the last pass's eta), the fused-pass workspace and a communicator.  A pass is
//   H2D beta -> irls_pass_kernel (one read of X) -> reduce_partials_kernel (fixed order)
//   -> [device all-reduce: RCCL over xGMI] -> D2H packed -> [host all-reduce callback]
// replacing one zwCreateBinomial + wlsComponents + treeReduce round of the reference
// (GLM.scala:453-458, utils.scala:110-126).
//
// This file: the engine's lifetime and workspace, pass / pass_dev / group_pass, the fused and
// narrow enqueue_pass, lm_device, stats, the external-backend adapter, and the ABI's handle, fit,
// irls_* and stats functions.  The rest of the engine and of the ABI:
//   comm.cpp         bounded waits, callbacks, the all-reduce helpers, sglm_set_comm*, sglm_local_comm
//   wide_path.cpp    wide designs (p > 256): schedules, the wide pass (enqueue_wide), the device solver
//   ingest.cpp       sglm_reserve / set_rows / set_data* / synth* / get_data / predict*
//   diagnostics.cpp  sglm_vcov / influence / vcov_robust / predict_new_se
//   vcov_cluster.cpp sglm_set_clusters / vcov_cluster / cluster_plan
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"
#include "solve.hpp"

using namespace sglm;

// Which kernel a pass runs (enum sglm_pass_kernel) and its name: the dispatch rules of
// ensure_workspace / launch_pass / launch_narrow / the wide path, in one place (the engine labels
// its passes with it; sglm_pass_kernel_for exposes it for a CPU test of the mapping).
static int pass_kernel_choice(int64_t n_pad, int P16, bool narrow, bool wide, bool proc, int fused_split, int family,
                              int link, char* name, size_t len) {
  static const char* fam[] = {"binomial", "gaussian", "poisson", "gamma", "negbin"};
  static const char* lnk[] = {"logit", "probit", "cloglog", "identity", "log", "inverse", "sqrt"};
  const char* f = (family >= 0 && family < 5) ? fam[family] : "?";
  // the link slot of the instantiation the launchers' dispatch picks (common.hpp dispatch_family_link):
  // the pairs without a dedicated one run their family's run-time-link instantiation
  const int il = dispatched_link(family, link);
  const char* l = il == LNK_RT ? "runtime" : (il >= 0 && il < 7) ? lnk[il] : "?";
  int k;
  if (wide) {
    k = proc ? SGLM_KERNEL_WIDE_PROC : SGLM_KERNEL_WIDE;
    std::snprintf(name, len, "wide_gram_kernel<%s>", proc ? "procedural" : "resident");
  } else if (narrow) {
    k = SGLM_KERNEL_NARROW;
    std::snprintf(name, len, "irls_narrow_kernel<%d,%s,%s>", P16, f, l);
  } else if (pass_uses_split(P16, fused_split, n_pad)) {
    k = SGLM_KERNEL_FUSED_SPLIT;
    std::snprintf(name, len, "irls_pass_r_kernel<%d,%s,%s>", P16, f, l);
  } else {
    k = SGLM_KERNEL_FUSED;
    std::snprintf(name, len, "irls_pass_kernel<%d,%s,%s>", P16, f, l);
  }
  return k;
}

// ---- lifetime and workspace ----
sglm_engine::~sglm_engine() {
  for (sglm_engine* s : subs) delete s;
  for (ncclComm_t c : gcomms)
    if (c) (void)ncclCommDestroy(c);
  subs.clear();
  gcomms.clear();
  release();
}

int sglm_engine::dev_alloc(double** ptr, size_t bytes, const char* what) {
  const hipError_t e = hipMalloc(ptr, bytes);
  if (e != hipSuccess) {
    *ptr = nullptr;
    (void)hipGetLastError();
    set_error(hip_msg(e, what));
    return SGLM_ENOMEM;
  }
  return SGLM_OK;
}

int sglm_engine::grow(double*& ptr, int64_t& cap, int64_t need, const char* what) {
  if (need <= cap) return SGLM_OK;
  if (ptr) HIPCHK(hipFree(ptr));
  ptr = nullptr;
  cap = 0;
  if (int rc = dev_alloc(&ptr, sizeof(double) * (size_t)need, what)) return rc;
  cap = need;
  return SGLM_OK;
}

void sglm_engine::dev_free(std::initializer_list<double**> ptrs) {
  for (double** ptr : ptrs) {
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
  }
}

void sglm_engine::free_data() {
  dev_free({&dX, &dy, &dm, &doff, &dprior, &deta, &dw, &dwz});
  n = p = n_pad = nblocks = 0;
  lm_last_pass_ms = -1.0;  // a new shard: the next device LM fit is timed
  rows_loaded = 0;
  written.clear();
  consts_family = -1;
  procx = ProcX{};
  dev_free({&dxsc, &dchunks});
  ch_rows = 0;
  nch = 0;
  proc_ov = false;
  nov = 0;
  ov_rows = 0;
  free_clusters(false);  // cluster ids belong to the rows they were declared for
  free_multinom();
}

void sglm_engine::release() {
  (void)hipSetDevice(device);
  free_data();
  dev_free({&dbeta, &dpart, &dred, &dsmall, &dgp, &drp, &dxs, &dvs, &dms, &dos});
  xs_cap = vs_cap = 0;
  dsmall_cap = 0;
  free_influence();
  free_clusters(true);
  for (int k = 0; k < 2; ++k) {
    if (hstage[k]) (void)hipHostFree(hstage[k]);
    if (evstage[k]) (void)hipEventDestroy(evstage[k]);
    hstage[k] = nullptr;
    evstage[k] = nullptr;
  }
  free_schedule();
  part_cap = red_cap = gp_cap = rp_cap = 0;
  if (blas) (void)rocblas_destroy_handle(blas);
  blas = nullptr;
  if (evm) (void)hipEventDestroy(evm);
  evm = nullptr;
  for (double** ptr : {&hbeta, &hred, &hsmall}) {
    if (*ptr) (void)hipHostFree(*ptr);
    *ptr = nullptr;
  }
  if (comm.nccl) (void)ncclCommDestroy(comm.nccl);
  comm.nccl = nullptr;
  for (hipEvent_t e : evchunk) (void)hipEventDestroy(e);
  evchunk.clear();
  if (st2) (void)hipStreamDestroy(st2);
  st2 = nullptr;
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  if (ev2) (void)hipEventDestroy(ev2);
  if (evpre) (void)hipEventDestroy(evpre);
  if (evc) (void)hipEventDestroy(evc);
  if (evt0) (void)hipEventDestroy(evt0);
  if (evt1) (void)hipEventDestroy(evt1);
  evt0 = evt1 = nullptr;
  if (st) (void)hipStreamDestroy(st);
  ev0 = ev1 = ev2 = evc = evpre = nullptr;
  st = nullptr;
}

int sglm_engine::ensure_small(int64_t count) {
  if (!hsmall) HIPCHK(hipHostMalloc(&hsmall, sizeof(double) * 64, hipHostMallocDefault));
  return grow(dsmall, dsmall_cap, std::max<int64_t>(64, count), "hipMalloc(small all-reduce buffer)");
}

// dred / hred hold at least len doubles (the packed result + the rank blocks of its scalars), and so
// do dbeta / hbeta
int sglm_engine::ensure_red_len(int64_t len) {
  if (len <= red_cap && dred) return SGLM_OK;
  if (dred) HIPCHK(hipFree(dred));
  if (hred) HIPCHK(hipHostFree(hred));
  dred = hred = nullptr;
  HIPCHK(hipMalloc(&dred, sizeof(double) * len));
  HIPCHK(hipHostMalloc(&hred, sizeof(double) * len, hipHostMallocDefault));
  if (dbeta) HIPCHK(hipFree(dbeta));
  if (hbeta) HIPCHK(hipHostFree(hbeta));
  dbeta = hbeta = nullptr;
  HIPCHK(hipMalloc(&dbeta, sizeof(double) * len));
  HIPCHK(hipHostMalloc(&hbeta, sizeof(double) * len, hipHostMallocDefault));
  red_cap = len;
  return SGLM_OK;
}

int sglm_engine::ensure_workspace() {
  if (wide) {
    P16 = 0;
    int rc = ensure_wide_workspace();
    if (rc) return rc;
  }
  narrow = !wide && p <= 64;
  if (narrow) {
    P16 = narrow_variant((int)p);
    stride = narrow_stride(P16);
    const int64_t want_grid = (int64_t)ncu * narrow_wg_per_cu();
    const int64_t per_wg = narrow_rows_per_wg(P16);
    const int64_t need = (nblocks * RB + per_wg - 1) / per_wg;
    grid = (int)std::max<int64_t>(1, std::min(need, want_grid));
  } else {
    if (!wide) P16 = pass_variant((int)p, fused_split, n_pad);
    stride = wide ? 0 : pass_stride(P16);
    if (!wide) {
      const int64_t want_grid = (int64_t)ncu * (pass_uses_split(P16, fused_split, n_pad) ? 1 : pass_wg_per_cu(P16));
      grid = (int)(nblocks < want_grid ? (nblocks > 0 ? nblocks : 1) : want_grid);
    }
  }
  const int64_t need_part = std::max<int64_t>((int64_t)grid * stride, 4096 * NS);
  if (int rc = grow(dpart, part_cap, need_part, "hipMalloc(pass partials)")) return rc;
  if (int rc = ensure_red_len(packed_len(p) + 16 * std::max(P16, 1))) return rc;
  return ensure_small(64);
}

int sglm_engine::alloc_data(int64_t n_, int64_t p_, bool has_m, bool has_off, bool has_prior, bool proc) {
  HIPCHK(hipSetDevice(device));
  free_data();
  if (n_ < 0 || p_ <= 0) {
    set_error("requirement failed: n >= 0 and p >= 1");
    return SGLM_EINVAL;
  }
  if (p_ > MAX_P_WIDE) {
    set_error("requirement failed: p <= " + std::to_string(MAX_P_WIDE) + " columns");
    return SGLM_EINVAL;
  }
  n = n_;
  p = p_;
  wide = force_wide || proc || p > 16 * MAX_P16;
  nblocks = (n + RB - 1) / RB;
  n_pad = std::max<int64_t>(nblocks, 1) * RB;
  const size_t vb = sizeof(double) * (size_t)n_pad;
  const size_t ncols = (size_t)((p + 7) / 8 * 8);  // whole column octets for the LDS-DMA staging
  hipError_t e = hipSuccess;
  if (!proc) {
    e = hipMalloc(&dX, vb * ncols);
    if (e != hipSuccess) {
      set_error(hip_msg(e, "hipMalloc(X)"));
      free_data();
      return SGLM_ENOMEM;
    }
    HIPCHK(hipMemsetAsync(dX, 0, vb * ncols, st));
  }
  for (auto pr : {std::make_pair(&dy, true), std::make_pair(&dm, has_m), std::make_pair(&doff, has_off),
                  std::make_pair(&dprior, has_prior), std::make_pair(&deta, true), std::make_pair(&dw, wide),
                  std::make_pair(&dwz, wide)}) {
    if (!pr.second) continue;
    e = hipMalloc(pr.first, vb);
    if (e != hipSuccess) {
      set_error(hip_msg(e, "hipMalloc(vector)"));
      free_data();
      return SGLM_ENOMEM;
    }
    HIPCHK(hipMemsetAsync(*pr.first, 0, vb, st));
  }
  return ensure_workspace();
}

// ---- Backend ----
int sglm_engine::global_sums(double* out2) {
  if (group()) {  // shard order, as the reference sums partitions (GLM.scala:420-423), compensated
    std::vector<double> blocks(2 * subs.size());
    for (size_t d = 0; d < subs.size(); ++d)
      if (int rc = subs[d]->global_sums(blocks.data() + 2 * d)) return rc;
    compensated_rank_sum(blocks.data(), (int)subs.size(), 2, out2);
    return SGLM_OK;
  }
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  const int nparts = 1024;
  HIPCHK(launch_ysum(dy, n, dpart, nparts, st));
  std::vector<double> h(nparts);
  HIPCHK(hipMemcpyAsync(h.data(), dpart, sizeof(double) * nparts, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  double s = 0.0, c = 0.0;
  for (int i = 0; i < nparts; ++i) neumaier_add(s, c, h[i]);
  out2[0] = s + c;
  out2[1] = (double)n;
  return allreduce_small(out2, 2);
}

int sglm_engine::pass_dev(int mode, const double* beta, double mu0, double ybar, int family, int link,
                          double* packed) {
  for (sglm_engine* s : shards()) s->dev_only = true;
  const int rc = pass(mode, beta, mu0, ybar, family, link, packed);
  for (sglm_engine* s : shards()) s->dev_only = false;
  dev_passes += 1;
  return rc;
}

int sglm_engine::pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) {
  if (int rc = theta_check(family)) return rc;
  if (group()) return group_pass(mode, beta, mu0, ybar, family, link, packed);
  const int64_t plen = packed_len(p), sc = tri_count(p) + p;
  const int R = gather_ranks() ? comm.nranks : 0;  // rank blocks of the scalars (compensated_rank_sum)
  const int64_t len = plen + (int64_t)NS * R;
  if (int rc = ensure_red_len(len)) return rc;
  int rc = enqueue_pass(mode, beta, mu0, ybar, family, link);
  if (rc) return rc;
  if (comm_on_device()) {
    if (R && (rc = stage_rank_block(comm.rank, R))) return rc;
    rc = allreduce_device(dred, len, true);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpyAsync(hred, dred, sizeof(double) * (comm_on_device() ? len : plen), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  rc = pass_timing();
  if (rc) return rc;
  red_on_device = comm_on_device() || comm.kind == 0;
  if (!comm_on_device()) {
    if (R) {
      std::fill(hred + plen, hred + len, 0.0);
      std::memcpy(hred + plen + (int64_t)comm.rank * NS, hred + sc, sizeof(double) * NS);
    }
    rc = allreduce_host(hred, comm.kind == 0 ? plen : len);
    if (rc) return rc;
  }
  if (R) compensated_rank_sum(hred + plen, R, NS, hred + sc);
  std::memcpy(packed, hred, sizeof(double) * plen);
  finish_scalars(mode, family, packed + sc);
  return SGLM_OK;
}

// The narrow pass's in-pass Poisson / Gamma statistics lack their per-fit constants (rowmath.hpp
// init_stats_const), which the fit's initial pass sums into S_AUX2: kept here, applied to every
// later pass that carried the statistics -- R's dpois loglik sum pw (y log mu - mu) minus
// sum pw lgamma(y + 1); Gamma's S_LL = sum pw log y and S_AUX1 = sum pw log mu = sum pw log y -
// sum pw log(y eta).  Applied once, on the all-reduced scalars.
// (The statistics ride only in passes of a fit, after its initial pass: enqueue_pass.)
void sglm_engine::finish_scalars(int mode, int family, double* s) {
  if (family != FAM_POISSON && family != FAM_GAMMA) return;
  if (mode == MODE_INIT_SINGLE || mode == MODE_INIT_MULTI) {
    stats_const = s[S_AUX2];
    s[S_AUX2] = 0.0;
    consts_family = family;
    for (sglm_engine* sub : subs) sub->consts_family = family;
    return;
  }
  if (mode != MODE_IRLS || !pass_has_stats()) return;
  if (family == FAM_POISSON) {
    s[S_LL] -= stats_const;
  } else {
    s[S_LL] = stats_const;
    s[S_AUX1] = stats_const - s[S_AUX1];
  }
}

// Kernel times of the pass just synchronised (HIP events on this engine's stream).
int sglm_engine::pass_timing() {
  float k1 = 0.f, k2 = 0.f;
  HIPCHK(hipEventElapsedTime(&k1, ev0, ev1));
  HIPCHK(hipEventElapsedTime(&k2, ev1, ev2));
  if (wide)
    if (int rc = wide_timing(k1)) return rc;
  passes += 1;
  pass_ms += k1;
  reduce_ms += k2;
  last_pass_ms = k1;
  last_reduce_ms = k2;
  return SGLM_OK;
}

// An untimed pass (enqueue_pass timed = false: LM.fit on the device, see lm_device) counts the
// kernel times of the last timed one.
void sglm_engine::pass_untimed() {
  passes += 1;
  pass_ms += lm_last_pass_ms;
  reduce_ms += lm_last_reduce_ms;
}

// H2D beta, the pass kernels and the fixed-order partial reduction into dred -- all
// asynchronous on this engine's stream (a multi-device handle enqueues every shard first).
int sglm_engine::enqueue_pass(int mode, const double* beta, double mu0, double ybar, int family, int link, bool timed) {
  HIPCHK(hipSetDevice(device));
  if (int rc = check_loaded()) return rc;
  if (beta) {
    std::memcpy(hbeta, beta, sizeof(double) * p);
    HIPCHK(hipMemcpyAsync(dbeta, hbeta, sizeof(double) * p, hipMemcpyHostToDevice, st));
  }
  PassArgs a{};
  a.X = dX;
  a.ld = n_pad;
  a.p = (int)p;
  a.nq = (int)((p + 3) / 4);
  a.y = dy;
  a.m = dm;
  a.off = doff;
  a.prior = dprior;
  a.beta = beta ? dbeta : nullptr;
  a.n = n;
  a.nblocks = nblocks;
  a.family = family;
  a.link = link;
  a.mode = mode;
  a.mu0 = mu0;
  a.ybar = ybar;
  a.partials = dpart;
  a.stride = stride;
  a.theta = theta;
  // Final statistics in the narrow pass, no eta store (rowmath.hpp stats_in_pass_family):
  // binomial / logit (m = 1) in every IRLS pass -- measured faster than the lean variant, the
  // statistics hide under the stream (DESIGN 4 K1') -- and Poisson / Gamma in the deviance-only
  // pass only, the pass glm_drive predicts to end the fit: at p = 64 their statistics rows cost
  // +14 % per pass (125M x 64 Poisson: 17.4 against 15.3 ms, tools/ab_stats.py; the family
  // arithmetic runs on 16 of 64 lanes there), while the deviance-only pass has no Gram to slow.
  // (Poisson / Gamma: only after this data's initial pass has summed the statistics' constants.)
  a.stats_in_pass = (narrow && mode == MODE_IRLS && stats_in_pass_family(family, link) &&
                     !(family == FAM_BINOMIAL && dm) &&
                     (family == FAM_BINOMIAL || (dev_only && consts_family == family)) && !want_eta) ? 1 : 0;
  if (meat_w) {
    // the sandwich's meat X' diag(omega) X (sglm_vcov_robust): a gaussian / identity pass at beta = 0
    // whose prior weights are omega; nothing of the shard's own vectors but y, no eta store, and the
    // fit's kernel record (sglm_stats.pass_kernel, pass_has_stats) stays what it was
    a.prior = meat_w;
    a.m = a.off = nullptr;
  } else {
    lp_stats = a.stats_in_pass != 0;
    note_kernel(mode == MODE_LM_GRAM ? FAM_GAUSSIAN : family, mode == MODE_LM_GRAM ? LNK_IDENTITY : link);
  }
  // the fixed-effects fits' effective offset o* = o + alpha_g (fe.cpp): the shard's own offset is never written
  if (off_override && !meat_w) a.off = off_override;
  a.eta_out = (mode == MODE_IRLS && !a.stats_in_pass && !meat_w) ? deta : nullptr;
  a.no_gram = dev_only ? 1 : 0;
  a.fused_split = fused_split;
  a.lm_extras = (mode == MODE_LM_GRAM && narrow && lm_extras_pass) ? 1 : 0;
  if (wide) return enqueue_wide(mode, beta != nullptr, mu0, ybar, family, link);  // wide_path.cpp
  // the pass kernel and the reduce record ev0 / ev1 / ev2 as part of their dispatches
  // (hipExtLaunchKernel): separate event records put a ~5 us marker between the kernels,
  // a tenth of an LM.fit on configs[0]
  hipEvent_t e0 = timed ? ev0 : nullptr, e1 = timed ? ev1 : nullptr, e2 = timed ? ev2 : nullptr;
  if (nblocks > 0) {
    if (narrow) HIPCHK(launch_narrow(P16, a, grid, st, e0, e1));
    else HIPCHK(launch_pass(P16, a, grid, st, e0, e1));
  } else {
    HIPCHK(hipEventRecord(ev0, st));
    HIPCHK(hipMemsetAsync(dpart, 0, sizeof(double) * stride, st));
    HIPCHK(hipEventRecord(ev1, st));
    e2 = ev2;
  }
  HIPCHK(launch_reduce(dpart, stride, nblocks > 0 ? grid : 1, (int)p, P16, dred, st, e2, a.lm_extras ? (int)p : 0));
  return SGLM_OK;
}

// The kernel this shard's passes run (sglm_stats.pass_kernel / pass_kernel_name): the engine's
// own dispatch decision -- narrow / fused / wide, and K1 against K1r by pass_uses_split with its
// row limit -- so a roofline line is labelled by what ran, not by a re-derived threshold.
void sglm_engine::note_kernel(int family, int link) {
  last_kernel = pass_kernel_choice(n_pad, P16, narrow, wide, procx.on != 0, fused_split, family, link,
                                   last_kernel_name, sizeof last_kernel_name);
}

// ---- multi-device handle: every shard's pass enqueued, then one reduction ----
// Distinct devices: ncclAllReduce of the packed buffers in one RCCL group call (xGMI), every
// shard ends with the sum.  Repeated devices (rehearsal on fewer GPUs): host sums in shard
// order.  Either way the wide-path device solver reads shard 0's buffers.
// The scalars are summed in shard order with compensation either way (compensated_rank_sum).
// comm_ms: RCCL -- the shortest span from a shard's pass end (ev2) to its all-reduce end (evc),
// i.e. the collective after the last shard arrived; host sums -- the host time of the sum.
int sglm_engine::group_pass(int mode, const double* beta, double mu0, double ybar, int family, int link,
                            double* packed) {
  const int64_t pp = subs[0]->p, plen = packed_len(pp), sc = tri_count(pp) + pp;
  const int D = (int)subs.size();
  const int64_t len = plen + (int64_t)NS * D;
  if (group_aborted) {
    set_error("the multi-device handle's RCCL group was aborted by an earlier failure; create a new handle");
    return SGLM_ECOMM;
  }
  for (sglm_engine* s : subs) {
    HIPCHK(hipSetDevice(s->device));
    if (int rc = s->ensure_red_len(len)) return rc;
  }
  for (sglm_engine* s : subs)
    if (int rc = s->enqueue_pass(mode, beta, mu0, ybar, family, link)) return rc;
  if (!gcomms.empty()) {
    for (int d = 0; d < D; ++d) {
      HIPCHK(hipSetDevice(subs[d]->device));
      if (int rc = subs[d]->stage_rank_block(d, D)) return rc;
    }
    ncclResult_t r = ncclGroupStart();
    for (int d = 0; d < D && r == ncclSuccess; ++d)
      r = ncclAllReduce(subs[d]->dred, subs[d]->dred, (size_t)len, ncclFloat64, ncclSum, gcomms[d], subs[d]->st);
    ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess) {
      set_error(std::string("RCCL ncclAllReduce (group): ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
      return SGLM_ECOMM;
    }
    for (sglm_engine* s : subs) {
      HIPCHK(hipSetDevice(s->device));
      HIPCHK(hipEventRecord(s->evc, s->st));
    }
    sglm_engine* s0 = subs[0];
    HIPCHK(hipSetDevice(s0->device));
    HIPCHK(hipMemcpyAsync(s0->hred, s0->dred, sizeof(double) * len, hipMemcpyDeviceToHost, s0->st));
    {  // every shard's stream drains, or the group is aborted at the deadline (wait_collective)
      std::vector<hipStream_t> sts;
      std::vector<ncclComm_t*> cs;
      std::vector<hipEvent_t> evs;  // every shard's pass done: the deadline starts there
      for (int d = 0; d < D; ++d) {
        sts.push_back(subs[d]->st);
        cs.push_back(&gcomms[d]);
        evs.push_back(subs[d]->ev2);
      }
      if (int rc = wait_collective(sts, cs, comm.timeout_ms, -1, "the multi-device ncclAllReduce group", evs)) {
        group_aborted = true;  // the handle's communicators are gone: every later pass fails
        return rc;
      }
    }
    double cms = -1.0;
    for (sglm_engine* s : subs) {
      HIPCHK(hipSetDevice(s->device));
      if (int rc = s->pass_timing()) return rc;
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, s->ev2, s->evc));
      cms = cms < 0.0 ? ms : std::min(cms, (double)ms);
    }
    comm.ms += std::max(cms, 0.0);
    compensated_rank_sum(s0->hred + plen, D, NS, s0->hred + sc);
    std::memcpy(packed, s0->hred, sizeof(double) * plen);
    s0->red_on_device = true;
  } else {
    for (sglm_engine* s : subs) {
      HIPCHK(hipSetDevice(s->device));
      HIPCHK(hipMemcpyAsync(s->hred, s->dred, sizeof(double) * plen, hipMemcpyDeviceToHost, s->st));
    }
    for (sglm_engine* s : subs) {
      HIPCHK(hipSetDevice(s->device));
      HIPCHK(hipStreamSynchronize(s->st));
      if (int rc = s->pass_timing()) return rc;
    }
    const double t0 = now_ms();
    std::memcpy(packed, subs[0]->hred, sizeof(double) * sc);
    for (int d = 1; d < D; ++d)
      for (int64_t k = 0; k < sc; ++k) packed[k] += subs[(size_t)d]->hred[k];
    std::vector<double> blocks((size_t)(NS * D));
    for (int d = 0; d < D; ++d) std::memcpy(blocks.data() + (int64_t)d * NS, subs[(size_t)d]->hred + sc, sizeof(double) * NS);
    compensated_rank_sum(blocks.data(), D, NS, packed + sc);
    subs[0]->red_on_device = false;
    comm.ms += now_ms() - t0;
  }
  finish_scalars(mode, family, packed + sc);
  return SGLM_OK;
}

// LM.fit in one round trip (driver.hpp Backend::lm_device): a resident narrow shard with no
// communicator -- the Gram pass, which also sums X'1 and y'y (narrow LMX), then lm_chol_kernel:
// the host Cholesky, bitwise, on the device, and the residual statistics of LM.scala:160-188 from
// those sums (SSE = y'y - 2 b'X'y + b'X'X b, ...; kernels.hip lm_chol_kernel), written with the
// whole result to pinned host memory -- ONE pass over X and one synchronisation.  Where the sums
// cancel too far (LM_ONEPASS_MAX_RATIO) the statistics come back flagged (S_BAD) and lm_drive runs
// the residual pass, the reference's own form; so does a device Cholesky that is not the host's.
// configs[0] (1M x 20) is launch- and latency-bound: round 5 removed the host round trip between
// the two passes, round 6 the second pass.
int sglm_engine::lm_device(double* packed, double* dev_coefs, double* s, bool& done) {
  done = false;
  if (!allow_lm_device || group() || comm.kind != 0 || wide || procx.on || !narrow || p > 64 || nblocks <= 0)
    return SGLM_OK;
  HIPCHK(hipSetDevice(device));
  // one device buffer, copied back in one piece: packed Gram | X'1 [p] | statistics [NS] | coefs [p]
  const int64_t plen = packed_len(p);
  if (int rc = ensure_red_len(plen + p + NS + p)) return rc;
  if (int rc = ensure_small(64)) return rc;
  // a kernel that carries a completion event ends ~4.5 us later than one that does not (its
  // end-of-kernel signal; measured on the configs[0] timeline): LM fits time their Gram pass on
  // every 16th fit and count that time for the others (pass_untimed)
  const bool timed = (lm_device_fits % 16) == 0 || lm_last_pass_ms < 0.0;
  lm_extras_pass = true;
  const int prc = enqueue_pass(MODE_LM_GRAM, nullptr, 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, timed);
  lm_extras_pass = false;
  if (prc) return prc;
  double* aux = dsmall + NS;  // {ybar, leave-Cholesky flag}
  double* dstat = dred + plen + p;
  double* dcoef = dred + plen + p + NS;
  double* hred_dev = nullptr;  // the pinned result buffer as the device sees it (no copy blit)
  HIPCHK(hipHostGetDevicePointer((void**)&hred_dev, hred, 0));
  LmOnePass op;
  op.x1 = dred + plen;
  op.stats = dstat;
  op.host = hred_dev;
  op.ncopy = plen + p;
  HIPCHK(launch_lm_chol(dred, (int)p, LU_SWITCH_RATIO, dcoef, aux, st, op));
  HIPCHK(hipStreamSynchronize(st));  // (a spin on hipStreamQuery measured slower: 0.124 against 0.115 ms)
  if (timed) {
    if (int rc = pass_timing()) return rc;
    lm_last_pass_ms = last_pass_ms;
    lm_last_reduce_ms = last_reduce_ms;
  } else {
    pass_untimed();
  }
  red_on_device = true;
  std::memcpy(packed, hred, sizeof(double) * plen);
  std::memcpy(s, hred + plen + p, sizeof(double) * NS);
  std::memcpy(dev_coefs, hred + plen + p + NS, sizeof(double) * p);
  done = true;
  lm_device_fits += 1;
  lm_onepass_fits += s[S_BAD] == 0.0 ? 1 : 0;
  return SGLM_OK;
}

int sglm_engine::stats(int mode, const double* beta, double mu0, double ybar, int family, int link, double* s) {
  if (int rc = theta_check(family)) return rc;
  if (group()) {  // shard order, compensated (compensated_rank_sum)
    std::vector<double> blocks((size_t)NS * subs.size());
    for (size_t d = 0; d < subs.size(); ++d)
      if (int rc = subs[d]->stats(mode, beta, mu0, ybar, family, link, blocks.data() + NS * d)) return rc;
    compensated_rank_sum(blocks.data(), (int)subs.size(), NS, s);
    return SGLM_OK;
  }
  HIPCHK(hipSetDevice(device));
  StatsArgs a{};
  // LM residuals of a narrow resident design: beta rides in the kernel arguments (no H2D copy on
  // the fit's critical path, configs[0] is launch- and latency-bound)
  const bool by_value = mode == MODE_LM_RESID && !procx.on && p <= STATS_BETA_MAX;
  if (mode == MODE_LM_RESID && !by_value) {  // pred = X * coefs into the eta buffer
    std::memcpy(hbeta, beta, sizeof(double) * p);
    HIPCHK(hipMemcpyAsync(dbeta, hbeta, sizeof(double) * p, hipMemcpyHostToDevice, st));
    if (procx.on) HIPCHK(launch_predict(dX, n_pad, (int)p, n, dbeta, nullptr, deta, st, procx));
  }
  if (mode == MODE_LM_RESID && !procx.on) {  // one read of X, no eta round trip
    a.X = dX;
    a.ld = n_pad;
    a.p = (int)p;
    a.beta = dbeta;
    a.beta_by_value = by_value ? 1 : 0;
    if (by_value) std::memcpy(a.bv, beta, sizeof(double) * p);
  }
  a.y = dy;
  a.m = (mode == MODE_LM_RESID) ? nullptr : dm;
  a.prior = (mode == MODE_LM_RESID) ? nullptr : dprior;
  a.eta = deta;
  a.n = n;
  a.family = family;
  a.link = link;
  a.mode = mode;
  a.mu0 = mu0;
  a.ybar = ybar;
  a.theta = theta;
  a.partials = dpart;
  // one wave per SIMD leaves the per-row chain latency-bound on large shards; small ones
  // (LM 1M x 20) keep 1024 partials; they are summed on the device (reduce_stats_kernel,
  // compensated) and only the NS sums come back
  const int nb = stats_blocks(n);
  HIPCHK(launch_stats(a, nb, st));
  if (int rc = ensure_small(64)) return rc;
  HIPCHK(launch_reduce_stats(dpart, nb, dsmall, st));
  HIPCHK(hipMemcpyAsync(hsmall, dsmall, sizeof(double) * NS, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(s, hsmall, sizeof(double) * NS);
  return allreduce_small(s, NS);
}

// =====================================================================================
// External backend adapter (caller-computed partials)
// =====================================================================================
namespace {

struct ExternalBackend : public Backend {
  const sglm_backend* be;
  sglm_allreduce_fn fn;
  void* ctx;
  int nranks = 1;
  int rank = -1;  // known for the in-process communicator: scalars then summed in rank blocks
  double timeout_ms = comm_timeout_ms_env();
  CallbackRunner runner;  // the callback on a communicator thread, waited for with the deadline
  ExternalBackend(const sglm_backend* b, sglm_allreduce_fn f, void* c) : be(b), fn(f), ctx(c), rank(known_rank(f, c)) {}
  int64_t ncols() const override { return be->p; }
  int npart() const override { return nranks; }
  int reduce_raw(double* buf, int64_t count) {
    return fn ? runner.call(fn, ctx, buf, count, nullptr, 0, timeout_ms, rank) : SGLM_OK;
  }
  // buf[0, count): the last nsc entries are scalar sums -- through rank blocks when the rank is known
  int reduce(double* buf, int64_t count, int64_t nsc) {
    if (!(fn && rank >= 0 && rank < nranks && nranks > 1)) return reduce_raw(buf, count);
    std::vector<double> b((size_t)(count + nsc * nranks), 0.0);
    std::memcpy(b.data(), buf, sizeof(double) * count);
    std::memcpy(b.data() + count + (int64_t)rank * nsc, buf + count - nsc, sizeof(double) * nsc);
    if (int rc = reduce_raw(b.data(), (int64_t)b.size())) return rc;
    std::memcpy(buf, b.data(), sizeof(double) * (count - nsc));
    compensated_rank_sum(b.data() + count, nranks, nsc, buf + count - nsc);
    return SGLM_OK;
  }
  int global_sums(double* out2) override {
    if (be->local_sums(be->ctx, out2) != 0) {
      set_error("external backend local_sums failed");
      return SGLM_EINVAL;
    }
    double one[1] = {1.0};
    int rc = reduce_raw(one, 1);  // counts the ranks joined by the communicator
    if (rc) return rc;
    nranks = (int)std::lround(one[0]);
    return reduce(out2, 2, 2);
  }
  int pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override {
    (void)family;
    (void)link;
    if (be->pass(be->ctx, mode, beta, mu0, ybar, packed) != 0) {
      set_error("external backend pass failed");
      return SGLM_EINVAL;
    }
    return reduce(packed, packed_len(be->p), NS);
  }
  int stats(int mode, const double* beta, double mu0, double ybar, int family, int link, double* s) override {
    std::vector<double> packed((size_t)packed_len(be->p));
    int rc = pass(mode, beta, mu0, ybar, family, link, packed.data());
    if (rc) return rc;
    std::memcpy(s, packed.data() + tri_count(be->p) + be->p, sizeof(double) * NS);
    return SGLM_OK;
  }
};

}  // namespace

// =====================================================================================
// C ABI: handles, fits, single passes, statistics
// =====================================================================================
extern "C" {

int sglm_abi_version(void) { return SGLM_ABI_VERSION; }
const char* sglm_last_error(void) { return get_error(); }

int sglm_device_count(int* count) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    set_error(hip_msg(e, "hipGetDeviceCount"));
    return SGLM_EHIP;
  }
  *count = c;
  return SGLM_OK;
}

int sglm_create_device(int device, sglm_engine** out) {
  if (!out) {
    set_error("requirement failed: out handle pointer");
    return SGLM_EINVAL;
  }
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    set_error(e != hipSuccess ? hip_msg(e, "hipGetDeviceCount") : std::string("no HIP device visible"));
    return SGLM_EHIP;
  }
  if (device < 0 || device >= count) {
    set_error("requirement failed: device ordinal out of range");
    return SGLM_EINVAL;
  }
  auto* h = new sglm_engine();
  h->device = device;
  auto fail = [&](hipError_t err, const char* what) {
    set_error(hip_msg(err, what));
    delete h;
    return SGLM_EHIP;
  };
  if ((e = hipSetDevice(device)) != hipSuccess) return fail(e, "hipSetDevice");
  if ((e = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipEventCreate(&h->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreate(&h->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreate(&h->ev2)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreate(&h->evc)) != hipSuccess) return fail(e, "hipEventCreate");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail(e, "hipGetDeviceProperties");
  h->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char* fw = std::getenv("SGLM_FORCE_WIDE")) h->force_wide = std::atoi(fw) != 0;
  if (const char* pc = std::getenv("SGLM_PROC_CHUNKS")) h->allow_chunks = std::atoi(pc) != 0;
  if (const char* po = std::getenv("SGLM_PROC_OVERLAP")) h->proc_ov_want = std::atoi(po);
  if (const char* pm = std::getenv("SGLM_PROC_OV_MIN")) h->proc_ov_min = std::max<int64_t>(32, std::atoll(pm));
  if (const char* ov = std::getenv("SGLM_WIDE_OVERLAP")) h->ov_want = std::atoi(ov);
  if (const char* om = std::getenv("SGLM_WIDE_OV_MIN")) h->ov_min = std::max<int64_t>(32, std::atoll(om));
  if (const char* sp = std::getenv("SGLM_SPECULATE")) h->allow_spec = std::atoi(sp) != 0;
  if (const char* ld = std::getenv("SGLM_LM_DEVICE")) h->allow_lm_device = std::atoi(ld) != 0;
  if (const char* fs = std::getenv("SGLM_FUSED_SPLIT")) h->fused_split = std::max(0, std::atoi(fs));
  if (const char* ws = std::getenv("SGLM_WIDE_SOLVE")) h->wide_lu = std::strcmp(ws, "lu") == 0;
  if (const char* pm = std::getenv("SGLM_PROC_SCRATCH_MAX")) h->proc_scratch_max = std::max<int64_t>(0, std::atoll(pm));
  *out = h;
  return SGLM_OK;
}

void sglm_destroy(sglm_engine* h) { delete h; }

// SURVEY 8(b)'s constructor: one handle over devs[0..ndev).  One device: the single-device handle
// (sglm_create_device); several: the group handle (sglm_create_multi).
int sglm_create(const int* devs, int ndev, sglm_engine** out) {
  if (!out || !devs || ndev < 1) {
    set_error("requirement failed: devs[ndev], ndev >= 1, out handle pointer");
    return SGLM_EINVAL;
  }
  *out = nullptr;
  return ndev == 1 ? sglm_create_device(devs[0], out) : sglm_create_multi(devs, ndev, out);
}

// The group handle: one shard engine per listed device, one RCCL communicator per device from
// ncclCommInitAll when they are distinct -- for one device too (a one-device group runs the RCCL
// group all-reduce path: the tests' way to execute it on a one-GPU box).
int sglm_create_multi(const int* devs, int ndev, sglm_engine** out) {
  if (!out || !devs || ndev < 1) {
    set_error("requirement failed: devs[ndev], ndev >= 1, out handle pointer");
    return SGLM_EINVAL;
  }
  *out = nullptr;
  auto* g = new sglm_engine();
  g->device = devs[0];
  for (int d = 0; d < ndev; ++d) {
    sglm_engine* s = nullptr;
    int rc = sglm_create_device(devs[d], &s);
    if (rc) {
      delete g;
      return rc;
    }
    g->subs.push_back(s);
  }
  g->allow_spec = g->subs[0]->allow_spec;  // the group handle drives the fit (SGLM_SPECULATE)
  bool distinct = true;
  for (int a = 0; a < ndev; ++a)
    for (int b = 0; b < a; ++b) distinct = distinct && devs[a] != devs[b];
  g->comm.timeout_ms = comm_timeout_ms_env();  // the group all-reduce's deadline (wait_collective)
  if (distinct) {  // one communicator per device, one process (ncclCommInitAll)
    g->gcomms.assign((size_t)ndev, nullptr);
    ncclResult_t r = ncclCommInitAll(g->gcomms.data(), ndev, devs);
    if (r != ncclSuccess) {
      g->gcomms.clear();
      set_error(std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
      delete g;
      return SGLM_ECOMM;
    }
  }
  *out = g;
  return SGLM_OK;
}

int sglm_handle_devices(sglm_engine* h, int* ndev) {
  if (int rc = check_handle(h)) return rc;
  *ndev = (int)h->shards().size();
  return SGLM_OK;
}

int sglm_fit_glm(sglm_engine* h, const sglm_glm_opts* opts, sglm_preglm* out) {
  if (int rc = check_handle(h)) return rc;
  if (!opts || !out || !out->coefs || !out->std_err) {
    set_error("requirement failed: opts, out, out->coefs, out->std_err");
    return SGLM_EINVAL;
  }
  if (int rc = check_ready(h)) return rc;
  return glm_drive(*h, *opts, out);
}

int sglm_fit_lm(sglm_engine* h, sglm_prelm* out) {
  if (int rc = check_handle(h)) return rc;
  if (!out || !out->coefs || !out->std_err) {
    set_error("requirement failed: out, out->coefs, out->std_err");
    return SGLM_EINVAL;
  }
  if (int rc = check_ready(h)) return rc;
  return lm_drive(*h, out);
}

int sglm_irls_pass(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double mu0, double* gram,
                   double* xtwz, double* scalars) {
  if (int rc = check_handle(h)) return rc;
  if (!opts || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link");
    return SGLM_EINVAL;
  }
  if (int rc = check_ready(h)) return rc;
  const int64_t p = h->ncols();
  std::vector<double> packed((size_t)packed_len(p)), g((size_t)(p * p)), x((size_t)p);
  const int mode = beta ? MODE_IRLS : (opts->init_mode == SGLM_INIT_MULTIPLE ? MODE_INIT_MULTI : MODE_INIT_SINGLE);
  int rc = h->pass(mode, beta, mu0, 0.0, opts->family, opts->link, packed.data());
  if (rc) return rc;
  unpack_gram(packed.data(), p, g.data(), x.data());
  if (gram) std::memcpy(gram, g.data(), sizeof(double) * g.size());
  if (xtwz) std::memcpy(xtwz, x.data(), sizeof(double) * x.size());
  if (scalars) std::memcpy(scalars, packed.data() + tri_count(p) + p, sizeof(double) * NS);
  return SGLM_OK;
}

int sglm_irls_step(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double* xtwx, double* xtwz,
                   double* dev) {
  if (!beta) {
    set_error("requirement failed: beta");
    return SGLM_EINVAL;
  }
  double s[NS];
  if (int rc = sglm_irls_pass(h, opts, beta, 0.0, xtwx, xtwz, s)) return rc;
  if (dev) *dev = family_dev_factor(opts->family) * s[S_DEV];
  return SGLM_OK;
}

int sglm_irls_iterations(sglm_engine* h, const sglm_glm_opts* opts, double* beta, int iters, double* last_dev) {
  if (int rc = check_handle(h)) return rc;
  if (!opts || !beta || iters < 0) {
    set_error("requirement failed: opts, beta, iters >= 0");
    return SGLM_EINVAL;
  }
  if (int rc = check_ready(h)) return rc;
  return irls_iterate(*h, *opts, beta, iters, last_dev);
}

int sglm_pass_kernel_for(int64_t n, int64_t p, int fused_split, int flags, int family, int link, char* name,
                         int64_t namelen) {
  if (n < 1 || p < 1 || fused_split < 0 || !family_link_valid(family, link)) {
    set_error("requirement failed: n >= 1, p >= 1, fused_split >= 0, a supported family/link");
    return -1;
  }
  const int64_t n_pad = (n + RB - 1) / RB * RB;  // alloc_data's leading dimension
  const bool proc = (flags & 1) != 0, wide = proc || (flags & 2) || p > 16 * MAX_P16, narrow = !wide && p <= 64;
  const int P16 = wide ? 0 : narrow ? narrow_variant((int)p) : pass_variant((int)p, fused_split, n_pad);
  char buf[64];
  const int k = pass_kernel_choice(n_pad, P16, narrow, wide, proc, fused_split, family, link, buf, sizeof buf);
  if (name && namelen > 0) std::snprintf(name, (size_t)namelen, "%s", buf);
  return k;
}

int sglm_get_stats(sglm_engine* h, sglm_stats* out) {
  if (int rc = check_handle(h)) return rc;
  if (h->group()) {  // kernel times: the slowest shard; rows and bytes: all shards
    if (int rc = sglm_get_stats(h->subs[0], out)) return rc;
    for (size_t d = 1; d < h->subs.size(); ++d) {
      sglm_stats s{};
      (void)sglm_get_stats(h->subs[d], &s);
      out->pass_kernel_ms = std::max(out->pass_kernel_ms, s.pass_kernel_ms);
      out->reduce_kernel_ms = std::max(out->reduce_kernel_ms, s.reduce_kernel_ms);
      out->last_pass_ms = std::max(out->last_pass_ms, s.last_pass_ms);
      out->row_kernel_ms = std::max(out->row_kernel_ms, s.row_kernel_ms);
      out->gram_kernel_ms = std::max(out->gram_kernel_ms, s.gram_kernel_ms);
      out->n_local += s.n_local;
      out->load_ms += s.load_ms;
      out->load_bytes += s.load_bytes;
    }
    out->pass_kernel_ms_min = out->pass_kernel_ms;
    for (size_t d = 1; d < h->subs.size(); ++d)
      out->pass_kernel_ms_min = std::min(out->pass_kernel_ms_min, h->subs[d]->pass_ms);
    out->comm_ms = h->comm.ms;
    out->solve_ms = h->solve_ms;
    out->ndev = (int)h->subs.size();
    out->rccl_group = h->gcomms.empty() ? 0 : 1;
    out->dev_passes = h->dev_passes;
    out->overlap_chunks = h->subs.empty() ? 0 : h->subs[0]->ov_chunks();
    out->comm_path = h->gcomms.empty() ? SGLM_COMM_GROUP_HOST : SGLM_COMM_GROUP_RCCL;
    out->rank_blocks = 1;
    out->solve_path = h->solve_path;
    return SGLM_OK;  // pass_kernel / pass_kernel_name: shard 0's (every shard runs the same variant)
  }
  out->passes = h->passes;
  out->pass_kernel_ms = h->pass_ms;
  out->reduce_kernel_ms = h->reduce_ms;
  out->last_pass_ms = h->last_pass_ms;
  out->comm_ms = h->comm.ms;
  out->solve_ms = h->solve_ms;
  out->n_local = h->n;
  out->p = h->p;
  out->workgroups = h->grid;
  out->kernel_variant = h->P16;
  out->path = h->wide ? 1 : (h->narrow ? 2 : 0);
  out->wide_panels = h->wide ? h->npan : 0;
  out->row_kernel_ms = h->row_ms;
  out->gram_kernel_ms = h->wide ? h->gram_ms : h->pass_ms;
  out->load_ms = h->load_ms;
  out->load_bytes = h->load_bytes;
  out->ndev = 1;
  out->rccl_group = 0;
  out->dev_passes = h->dev_passes;
  out->overlap_chunks = h->ov_chunks();
  out->comm_path = h->comm.kind == 2   ? SGLM_COMM_RCCL
                   : h->comm.kind == 1 ? (h->comm.on_device ? SGLM_COMM_CALLER_DEVICE : SGLM_COMM_CALLER_HOST)
                                       : SGLM_COMM_NONE;
  out->rank_blocks = h->gather_ranks() ? 1 : 0;
  out->pass_kernel_ms_min = h->pass_ms;
  out->proc_chunks = h->nch;
  out->proc_chunk_rows = h->ch_rows;
  out->solve_path = h->solve_path;
  out->pass_kernel = h->last_kernel;
  out->lm_device_fits = h->lm_device_fits;
  out->lm_device_reruns = h->lm_device_reruns;
  out->lm_onepass_fits = h->lm_onepass_fits;
  std::memcpy(out->pass_kernel_name, h->last_kernel_name, sizeof out->pass_kernel_name);
  return SGLM_OK;
}

int sglm_reset_stats(sglm_engine* h) {
  if (int rc = check_handle(h)) return rc;
  for (sglm_engine* s : h->subs) (void)sglm_reset_stats(s);
  h->passes = h->dev_passes = h->lm_device_fits = h->lm_device_reruns = h->lm_onepass_fits = 0;
  h->pass_ms = h->reduce_ms = h->last_pass_ms = h->last_reduce_ms = h->row_ms = h->gram_ms = 0.0;
  h->comm.ms = 0.0;
  h->solve_ms = 0.0;
  h->load_ms = 0.0;
  h->load_bytes = 0;
  return SGLM_OK;
}

int sglm_fit_glm_external(const sglm_backend* be, sglm_allreduce_fn fn, void* comm_ctx, const sglm_glm_opts* opts,
                          sglm_preglm* out) {
  if (!be || !be->pass || !be->local_sums || be->p <= 0 || !opts || !out || !out->coefs || !out->std_err) {
    set_error("requirement failed: backend callbacks, p >= 1, opts, out");
    return SGLM_EINVAL;
  }
  if (opts->family == FAM_NEGBIN) {  // the pass callback has no theta to take
    set_error("requirement failed: the negative binomial family is not available over an external backend "
              "(sglm_backend.pass carries no theta)");
    return SGLM_EINVAL;
  }
  ExternalBackend eb(be, fn, comm_ctx);
  return glm_drive(eb, *opts, out);
}

int sglm_fit_lm_external(const sglm_backend* be, sglm_allreduce_fn fn, void* comm_ctx, sglm_prelm* out) {
  if (!be || !be->pass || !be->local_sums || be->p <= 0 || !out || !out->coefs || !out->std_err) {
    set_error("requirement failed: backend callbacks, p >= 1, out");
    return SGLM_EINVAL;
  }
  ExternalBackend eb(be, fn, comm_ctx);
  double sums[2];
  if (int rc = eb.global_sums(sums)) return rc;  // establishes the rank count
  return lm_drive(eb, out);
}

}  // extern "C"
