// vcov_cluster.cpp -- the cluster-robust covariance V = a C M C (sandwich::vcovCL; sglm_vcov_cluster): the
// cluster ids of the resident rows and their segments (sglm_set_clusters, sglm_cluster_plan), the
// cluster sums S of cluster.hip, their sum over shards and ranks, and the meat M = S'S from the
// tuned Gram pass of an internal engine whose design is S.
#include <algorithm>
#include <cstring>
#include <limits>

#include "engine.hpp"

using namespace sglm;

void sglm_engine::free_clusters(bool inner_too) {
  if (dclidx) (void)hipFree(dclidx);
  dclidx = nullptr;
  dev_free({&dR, &dP});
  free_fe();
  free_fe2();
  free_gee();
  cl_levels.clear();
  cl_G = 0;
  cl_nseg = cl_ntiles = 0;
  cl_S_stale = true;
  if (!inner_too) return;
  delete cl_inner;
  cl_inner = nullptr;
  for (hipEvent_t& e : evcl) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

// The combine's plan (engine.hpp): level by level, the open ranges cut into chunks
int64_t sglm::plan_combine(std::vector<CombineRange> cur, std::vector<int64_t>& idx,
                           std::vector<sglm_engine::CombineLevel>& levels) {
  std::vector<CombineRange> next;
  int64_t prow = 0;  // rows of the scratch handed out so far (a level reads the rows the one before wrote)
  int64_t in_row = -1;
  while (!cur.empty()) {
    sglm_engine::CombineLevel lv{};
    lv.start_off = (int64_t)idx.size();
    lv.in_row = in_row;
    lv.out_row = prow;
    std::vector<int64_t> dst;
    next.clear();
    int64_t out = 0;
    for (const CombineRange& r : cur) {
      const int64_t nch = (r.hi - r.lo + CLUSTER_CHUNK - 1) / CLUSTER_CHUNK;
      if (nch > 1) next.push_back({r.dst, out, out + nch});
      for (int64_t c = 0; c < nch; ++c) {
        idx.push_back(r.lo + c * CLUSTER_CHUNK);
        dst.push_back(nch == 1 ? r.dst : -(out++ + 1));
      }
    }
    idx.push_back(cur.back().hi);
    lv.nchunk = (int64_t)dst.size();
    lv.dst_off = (int64_t)idx.size();
    idx.insert(idx.end(), dst.begin(), dst.end());
    levels.push_back(lv);
    in_row = prow;
    prow += out;
    cur.swap(next);
  }
  return prow;
}

int sglm::combine_levels(sglm_engine* s, const std::vector<sglm_engine::CombineLevel>& levels, const int64_t* base,
                         const int64_t* idx0, const double* R, double* P, int ncol, double* S, int64_t ldS,
                         hipEvent_t e0, hipEvent_t e1) {
  for (size_t l = 0; l < levels.size(); ++l) {
    const sglm_engine::CombineLevel& lv = levels[l];
    CombineArgs c{};
    c.in = l == 0 ? R : P + lv.in_row * ncol;
    c.idx = l == 0 ? idx0 : nullptr;
    c.chunk_start = base + lv.start_off;
    c.chunk_dst = base + lv.dst_off;
    c.nchunk = lv.nchunk;
    c.p = ncol;
    c.S = S;
    c.ldS = ldS;
    c.out = P ? P + lv.out_row * ncol : nullptr;
    HIPCHK(launch_cluster_combine(c, s->ncu, s->st, l == 0 ? e0 : nullptr, l + 1 == levels.size() ? e1 : nullptr));
  }
  return SGLM_OK;
}

int sglm_engine::combine_clusters(const double* R, double* P, int ncol, double* S, int64_t ldS, hipEvent_t e0,
                                  hipEvent_t e1) {
  return combine_levels(this, cl_levels, dclidx, cl_seg(), R, P, ncol, S, ldS, e0, e1);
}

// The segments of this shard's rows under ids, the combine's levels over their CSR by cluster, and
// the buffers of the segment sums and of the combine's partial sums.
int sglm_engine::set_clusters_local(const int32_t* ids, int64_t nl, int32_t G) {
  HIPCHK(hipSetDevice(device));
  free_clusters(false);
  if (!ids) return SGLM_OK;
  if (nl != n) {
    set_error("requirement failed: " + std::to_string(nl) + " cluster ids for " + std::to_string(n) + " resident rows");
    return SGLM_EINVAL;
  }
  const int64_t nseg = cluster_segments(ids, n, G, nullptr, nullptr);
  if (nseg < 0) {
    set_error("requirement failed: every cluster id in [0, G = " + std::to_string(G) + ")");
    return SGLM_EINVAL;
  }
  const int64_t ntiles = (n + CLUSTER_TILE_ROWS - 1) / CLUSTER_TILE_ROWS;
  // seg_start [nseg + 2] | tile_seg [ntiles + 1] | cl_seg [nseg] | the levels' chunk_start, chunk_dst | seg_cluster [nseg]
  std::vector<int64_t> idx((size_t)(nseg + 2 + ntiles + 1 + nseg));
  std::vector<int32_t> seg_cl((size_t)nseg);
  std::vector<int64_t> cl_ptr((size_t)G + 1, 0);
  {
    int64_t* start = idx.data();
    int64_t* tile = start + nseg + 2;
    int64_t* by_cluster = tile + ntiles + 1;
    (void)cluster_segments(ids, n, G, start, seg_cl.data());
    start[nseg + 1] = std::numeric_limits<int64_t>::max();  // never a row: the walk past the last segment
    for (int64_t k = 0; k < nseg; ++k)
      if (start[k] % CLUSTER_TILE_ROWS == 0) tile[start[k] / CLUSTER_TILE_ROWS] = k;
    tile[ntiles] = nseg;
    // segments stably ordered by cluster: a cluster's segments in row order
    for (int64_t k = 0; k < nseg; ++k) cl_ptr[(size_t)seg_cl[(size_t)k] + 1] += 1;
    for (int32_t g = 0; g < G; ++g) cl_ptr[(size_t)g + 1] += cl_ptr[(size_t)g];
    std::vector<int64_t> at(cl_ptr.begin(), cl_ptr.end() - 1);
    for (int64_t k = 0; k < nseg; ++k) by_cluster[at[(size_t)seg_cl[(size_t)k]]++] = k;
  }
  // the combine's levels: at level 0 a cluster owns the CSR positions of its segments
  std::vector<CombineRange> open;
  for (int32_t g = 0; g < G; ++g)
    if (cl_ptr[(size_t)g + 1] > cl_ptr[(size_t)g]) open.push_back({g, cl_ptr[(size_t)g], cl_ptr[(size_t)g + 1]});
  const int64_t prow = plan_combine(std::move(open), idx, cl_levels);
  cl_segcl_off = (int64_t)idx.size();  // seg_cluster [nseg]: the fixed-effects offset kernel's (fe.hip)
  idx.insert(idx.end(), seg_cl.begin(), seg_cl.end());
  cl_prow = prow;
  hipError_t e = hipMalloc(&dclidx, sizeof(int64_t) * idx.size());
  if (e == hipSuccess) e = hipMalloc(&dR, sizeof(double) * (size_t)std::max<int64_t>(nseg * p, 1));
  if (e == hipSuccess && prow > 0) e = hipMalloc(&dP, sizeof(double) * (size_t)(prow * p));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    free_clusters(false);
    set_error(hip_msg(e, "hipMalloc(cluster segment sums)") + ": " + std::to_string(nseg) + " segments of " +
              std::to_string(p) + " doubles for " + std::to_string(n) + " rows -- sort the rows by cluster, so that a "
              "cluster's rows are consecutive (segments: runs of one id, about G + n / " +
              std::to_string(CLUSTER_TILE_ROWS) + " when sorted, n when interleaved)");
    return SGLM_ENOMEM;
  }
  HIPCHK(hipMemcpy(dclidx, idx.data(), sizeof(int64_t) * idx.size(), hipMemcpyHostToDevice));
  cl_G = G;
  cl_nseg = nseg;
  cl_ntiles = ntiles;
  return SGLM_OK;
}

// u_i = w_i (y_i - mu_i) g'(mu_i) of this shard's rows at beta into domega, zeros on the padding rows:
// enqueued on the stream, timed by evi0 / evi1
int sglm_engine::uscore_local(const double* beta, int family, int link) {
  HIPCHK(hipSetDevice(device));
  for (hipEvent_t& e : evcl)
    if (!e) HIPCHK(hipEventCreate(&e));
  return rows_enqueue(INFL_USCORE, beta, nullptr, family, link, InflArgs{}, true);
}

// The internal engine on this device whose design is the G x p matrix of cluster sums
int sglm_engine::ensure_cl_inner() {
  HIPCHK(hipSetDevice(device));
  if (!cl_inner)
    if (int rc = sglm_create_device(device, &cl_inner)) return rc;
  if (cl_inner->n != cl_G || cl_inner->p != p) {
    if (int rc = cl_inner->alloc_data(cl_G, p, false, false, false)) return rc;
    cl_inner->rows_loaded = cl_G;
    cl_inner->written.assign(1, std::make_pair((int64_t)0, (int64_t)cl_G));
    HIPCHK(hipStreamSynchronize(cl_inner->st));  // its zero fill, before this stream writes S there
  }
  return SGLM_OK;
}

// Segment sums of u x, then the cluster sums S into the internal engine's design: enqueued on the
// stream after uscore_local
int sglm_engine::cluster_sums_local() {
  if (int rc = ensure_cl_inner()) return rc;
  // The combine rewrites the rows of the clusters that have a segment on this shard and no others.  The
  // rest must be zero: S is cleared after new ids, and after every call whose cross-shard sum was
  // written into it (sglm_vcov_cluster marks it) -- a lone shard's S keeps its zero rows from call to call.
  if (cl_S_stale) {
    HIPCHK(hipMemsetAsync(cl_inner->dX, 0, sizeof(double) * (size_t)cluster_len(), st));
    cl_S_stale = false;
  }
  ClusterArgs a{};
  a.X = dX;
  a.ld = n_pad;
  a.p = (int)p;
  a.n = n;
  a.u = domega;
  a.seg_start = seg_start();
  a.tile_seg = tile_seg();
  a.ntiles = cl_ntiles;
  a.R = dR;
  HIPCHK(launch_cluster_sum(a, cluster_sum_grid(ncu, n, (int)p), st, evcl[0], evcl[1]));
  return combine_clusters(dR, dP, (int)p, cl_inner->dX, cl_inner->n_pad, evcl[2], evcl[3]);
}

int sglm_engine::cluster_sync() {
  if (int rc = rows_sync(&cl_ms[0])) return rc;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, evcl[0], evcl[1]));
  cl_ms[1] = ms;
  cl_ms[2] = 0.0;
  if (!cl_levels.empty()) {  // (no level, no combine launch: its events were not recorded)
    HIPCHK(hipEventElapsedTime(&ms, evcl[2], evcl[3]));
    cl_ms[2] = ms;
  }
  return SGLM_OK;
}

// S summed over the handle's shards or ranks, a plain sum that leaves every rank (a group: shard 0)
// with bitwise the same S: the group's RCCL all-reduce or its host sum in shard order, the engine's
// RCCL communicator, or the caller's all-reduce on device or host buffers.
int sglm::sum_cluster_scores(sglm_engine* h, const std::function<double*(sglm_engine*)>& buf, int64_t len) {
  const std::vector<sglm_engine*>& shards = h->shards();
  sglm_engine* s0 = shards[0];
  if (h->group()) {
    const int D = (int)shards.size();
    if (!h->gcomms.empty()) {
      ncclResult_t r = ncclGroupStart();
      for (int d = 0; d < D && r == ncclSuccess; ++d)
        r = ncclAllReduce(buf(shards[d]), buf(shards[d]), (size_t)len, ncclFloat64, ncclSum, h->gcomms[d],
                          shards[d]->st);
      const ncclResult_t r2 = ncclGroupEnd();
      if (r != ncclSuccess || r2 != ncclSuccess) {
        set_error(std::string("RCCL ncclAllReduce (group, cluster sums): ") +
                  ncclGetErrorString(r != ncclSuccess ? r : r2));
        return SGLM_ECOMM;
      }
      std::vector<hipStream_t> sts;
      std::vector<ncclComm_t*> cs;
      for (int d = 0; d < D; ++d) {
        sts.push_back(shards[d]->st);
        cs.push_back(&h->gcomms[d]);
      }
      if (int rc = wait_collective(sts, cs, h->comm.timeout_ms, -1, "the multi-device ncclAllReduce group")) {
        h->group_aborted = true;
        return rc;
      }
      return SGLM_OK;
    }
    const double t0 = now_ms();
    std::vector<double> sum((size_t)len), part((size_t)len);
    for (int d = 0; d < D; ++d) {
      HIPCHK(hipSetDevice(shards[d]->device));
      HIPCHK(hipMemcpy(d == 0 ? sum.data() : part.data(), buf(shards[d]), sizeof(double) * len,
                       hipMemcpyDeviceToHost));
      if (d > 0)
        for (int64_t k = 0; k < len; ++k) sum[(size_t)k] += part[(size_t)k];
    }
    HIPCHK(hipSetDevice(s0->device));
    HIPCHK(hipMemcpy(buf(s0), sum.data(), sizeof(double) * len, hipMemcpyHostToDevice));
    h->comm.ms += now_ms() - t0;
    return SGLM_OK;
  }
  if (h->comm.kind == 0) return SGLM_OK;
  HIPCHK(hipSetDevice(h->device));
  if (h->comm_on_device()) {
    if (int rc = h->allreduce_device(buf(h), len)) return rc;
    HIPCHK(hipStreamSynchronize(h->st));
    return SGLM_OK;
  }
  std::vector<double> host((size_t)len);
  HIPCHK(hipMemcpy(host.data(), buf(h), sizeof(double) * len, hipMemcpyDeviceToHost));
  if (int rc = h->allreduce_host(host.data(), len)) return rc;
  HIPCHK(hipMemcpy(buf(h), host.data(), sizeof(double) * len, hipMemcpyHostToDevice));
  return SGLM_OK;
}

// Every shard of the handle declared the same number of clusters, and so did every rank of its
// communicator (one small all-reduce: collective), or every rank fails.
int sglm::cluster_count(sglm_engine* h, int32_t* Gout) {
  const std::vector<sglm_engine*>& shards = h->shards();
  int32_t G = shards[0]->cl_G;
  for (const sglm_engine* s : shards) G = s->cl_G == G ? G : 0;
  if (!h->group() && h->comm.kind != 0) {
    // every rank declared the same G, or every rank fails: G = 65536 a + b, and the values a_r are all
    // equal iff R sum a_r^2 = (sum a_r)^2 (every term exact in fp64); a rank without clusters joins with 0
    const double a = (double)(G >> 16), b = (double)(G & 0xffff);
    double v[5] = {1.0, a, a * a, b, b * b};
    if (int rc = h->allreduce_small(v, 5)) return rc;
    if (v[0] * v[2] != v[1] * v[1] || v[0] * v[4] != v[3] * v[3]) {
      set_error("requirement failed: every rank of the communicator declares the same number of clusters G "
                "(sglm_set_clusters; this rank: " + std::to_string(G) + ")");
      return SGLM_EINVAL;
    }
  }
  if (G < 1) {
    set_error("requirement failed: cluster ids of the resident rows (sglm_set_clusters; a call that replaces the "
              "data drops them)");
    return SGLM_EINVAL;
  }
  *Gout = G;
  return SGLM_OK;
}

int sglm::check_cluster_hc(int hc_type) {
  if (hc_type == SGLM_HC0 || hc_type == SGLM_HC1) return SGLM_OK;
  set_error("requirement failed: hc_type SGLM_HC0 or SGLM_HC1 under clustering (HC2 / HC3 need per-cluster "
            "leverage blocks, which the engine does not form)");
  return SGLM_EINVAL;
}

int sglm::check_cadjust(int cadjust, int32_t G) {
  if (!cadjust || G >= 2) return SGLM_OK;
  set_error("requirement failed: cadjust (the factor G / (G - 1)) needs G >= 2 clusters");
  return SGLM_EINVAL;
}

int sglm::clustered_finish(int hc_type, double nrows, int64_t p, int64_t absorbed, int32_t G, int cadjust,
                           const std::vector<double>& C, const std::vector<double>& M, const char* at, double* cov,
                           double* meat) {
  double f = hc_type == SGLM_HC1 ? (nrows - 1.0) / (nrows - (double)p - (double)absorbed) : 1.0;
  if (cadjust) f *= (double)G / ((double)G - 1.0);
  if (!sandwich_product(C, M, p, f, cov)) {
    set_error(std::string("requirement failed: the cluster-robust covariance is not finite (a row whose mean leaves "
                          "the family's range at ") + at + ")");
    return SGLM_EINVAL;
  }
  if (meat) std::memcpy(meat, M.data(), sizeof(double) * M.size());
  return SGLM_OK;
}

extern "C" {

int sglm_cluster_plan(const int32_t* ids, int64_t n, int32_t G, int64_t* tile_rows, int64_t* nseg, int64_t* seg_start,
                      int32_t* seg_cluster) {
  if (n < 0 || G < 0 || (n > 0 && !ids)) {
    set_error("requirement failed: n >= 0, G >= 0, ids [n]");
    return SGLM_EINVAL;
  }
  if (tile_rows) *tile_rows = CLUSTER_TILE_ROWS;
  const int64_t k = cluster_segments(ids, n, G, seg_start, seg_cluster);
  if (k < 0) {
    set_error("requirement failed: every cluster id in [0, G = " + std::to_string(G) + ")");
    return SGLM_EINVAL;
  }
  if (nseg) *nseg = k;
  return SGLM_OK;
}

int sglm_set_clusters(sglm_engine* h, const int32_t* ids, int64_t n_local, int32_t G) {
  if (int rc = check_handle(h)) return rc;
  if (!ids) {  // clears
    for (sglm_engine* s : h->shards()) s->free_clusters(false);
    return SGLM_OK;
  }
  if (int rc = check_ready(h)) return rc;
  const int64_t rows = h->group() ? h->g_n : h->n;
  if (G < 1 || n_local != rows) {
    set_error("requirement failed: G >= 1 and n_local = the handle's " + std::to_string(rows) + " resident rows (got " +
              std::to_string(n_local) + ")");
    return SGLM_EINVAL;
  }
  const std::vector<sglm_engine*>& shards = h->shards();
  for (size_t d = 0; d < shards.size(); ++d) {
    const int64_t lo = h->group() ? h->sub_lo[d] : 0;
    if (int rc = shards[d]->set_clusters_local(ids + lo, shards[d]->n, G)) {
      for (sglm_engine* s : shards) s->free_clusters(false);
      return rc;
    }
  }
  return SGLM_OK;
}

int sglm_vcov_cluster(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, int hc_type, int cadjust,
                      double* cov, double* meat) {
  if (!opts || !beta || !cov || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link, beta, cov");
    return SGLM_EINVAL;
  }
  if (int rc = check_cluster_hc(hc_type)) return rc;
  if (int rc = check_handle(h)) return rc;
  if (int rc = check_ready(h)) return rc;
  if (int rc = require_fused_or_narrow(h, "the cluster-robust covariance needs")) return rc;
  if (h->group() && h->group_aborted) {
    set_error("the multi-device handle's RCCL group was aborted by an earlier failure; create a new handle");
    return SGLM_ECOMM;
  }
  int32_t G = 0;
  if (int rc = cluster_count(h, &G)) return rc;
  if (int rc = check_cadjust(cadjust, G)) return rc;
  const std::vector<sglm_engine*>& shards = h->shards();
  const int64_t p = h->ncols();
  std::vector<double> C((size_t)(p * p)), M((size_t)(p * p)), x((size_t)p);
  if (int rc = vcov_impl(h, opts, beta, C.data())) return rc;
  for (sglm_engine* s : shards) {
    if (int rc = s->uscore_local(beta, opts->family, opts->link)) return rc;
    if (int rc = s->cluster_sums_local()) return rc;
  }
  for (sglm_engine* s : shards)
    if (int rc = s->cluster_sync()) return rc;
  // the sum over shards or ranks lands in S itself: rows of clusters that have no segment on a shard
  // then hold other shards' sums, which this shard's next combine would not rewrite
  if (h->group() || h->comm.kind != 0)
    for (sglm_engine* s : shards) s->cl_S_stale = true;
  if (int rc = sum_cluster_scores(h, [](sglm_engine* s) { return s->cl_inner->dX; }, shards[0]->cluster_len())) return rc;
  // M = S'S: the LM Gram pass of the internal engine over S -- every rank from the identical S
  sglm_engine* in = shards[0]->cl_inner;
  std::vector<double> packed((size_t)packed_len(p));
  if (int rc = in->pass(MODE_LM_GRAM, nullptr, 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, packed.data())) return rc;
  unpack_gram(packed.data(), p, M.data(), x.data());
  for (int k = 0; k < 3; ++k) h->cl_ms[k] = slowest_shard(h, [k](const sglm_engine* s) { return s->cl_ms[k]; });
  h->cl_ms[3] = in->last_pass_ms;
  double nrows = (double)(h->group() ? h->g_n : h->n);  // HC1: every row of every shard, weight 0 included
  if (hc_type == SGLM_HC1 && !h->group())
    if (int rc = h->allreduce_small(&nrows, 1)) return rc;
  return clustered_finish(hc_type, nrows, p, 0, G, cadjust, C, M, "beta", cov, meat);
}

int sglm_get_cluster_ms(sglm_engine* h, double* score_ms, double* sum_ms, double* combine_ms, double* gram_ms) {
  if (int rc = check_handle(h)) return rc;
  if (!score_ms || !sum_ms || !combine_ms || !gram_ms) {
    set_error("requirement failed: score_ms, sum_ms, combine_ms, gram_ms");
    return SGLM_EINVAL;
  }
  *score_ms = h->cl_ms[0];
  *sum_ms = h->cl_ms[1];
  *combine_ms = h->cl_ms[2];
  *gram_ms = h->cl_ms[3];
  return SGLM_OK;
}

}  // extern "C"
