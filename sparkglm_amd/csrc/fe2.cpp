// fe2.cpp -- two-way fixed-effects GLM fits: a second absorbed factor beside the cluster factor
// (sglm_set_fe2, sglm_fe2_plan, sglm_fit_glm_fe2, sglm_fe2_pass, sglm_vcov_fe2; fixest::feglm with two factors;
// DESIGN.md 4, K12).
//
// One step at (beta, alpha, gamma): o* = offset + alpha_g + gamma_h (fe2_offset_kernel); an ordinary pass that
// reads o* and stores eta; the one-way step's weights kernel and segment sums give w and S1 | t1 | W1 over
// factor 1 (fe.cpp) and leave w z per row beside w; fe2_list_sum_kernel sums [w x | w z | w] into S2 | t2 | W2
// over factor 2's row lists, joined by the combine tree (vcov_cluster.cpp's planner and launcher); block
// Gauss-Seidel sweeps on the level coefficients Y = [a ; c] (fe2_gather_kernel + combine + fe2_update_kernel
// per half sweep) until the largest column-wise relative change is below the tolerance; the cross product
// S_X' Y on fp64 MFMA (fe2_cross_kernel), symmetrised on the host, and the downdate [A | b] = X'W[X | z] - S_X' Y.  The fit is glm_drive over a Backend whose pass is
// this step; the effects move by alpha += a_z - a_X beta+, gamma += c_z - c_X beta+ at the start of the next
// pass and are normalised per connected component of the level graph.  No second copy of X is made.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

#include "engine.hpp"

using namespace sglm;

namespace {

// The host's plan for two factors: the row list of factor 2, its chunks, and the components of the level graph
struct Fe2Plan {
  std::vector<int64_t> list;         // [n] rows ordered by factor-2 code, ascending within a code
  std::vector<int64_t> chunk_start;  // [nchunk + 1] positions in list
  std::vector<int32_t> chunk_level;  // [nchunk]
  std::vector<int32_t> comp1, comp2; // component of each level, -1: no rows
  std::vector<int32_t> low;          // [ncomp] lowest factor-2 code of each component, ascending
  std::vector<int32_t> nlev2;        // [ncomp] factor-2 levels (with rows) of each component
};

// false: a code outside [0, G) x [0, H)
bool fe2_plan(const int32_t* ids1, const int32_t* ids2, int64_t n, int32_t G, int32_t H, Fe2Plan& pl) {
  for (int64_t i = 0; i < n; ++i)
    if (ids1[i] < 0 || ids1[i] >= G || ids2[i] < 0 || ids2[i] >= H) return false;
  // stable counting sort of the rows by factor-2 code
  std::vector<int64_t> ptr((size_t)H + 1, 0);
  for (int64_t i = 0; i < n; ++i) ptr[(size_t)ids2[i] + 1] += 1;
  for (int32_t h = 0; h < H; ++h) ptr[(size_t)h + 1] += ptr[(size_t)h];
  pl.list.assign((size_t)n, 0);
  {
    std::vector<int64_t> at(ptr.begin(), ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) pl.list[(size_t)at[(size_t)ids2[i]]++] = i;
  }
  pl.chunk_start.clear();
  pl.chunk_level.clear();
  for (int32_t h = 0; h < H; ++h)
    for (int64_t q = ptr[(size_t)h]; q < ptr[(size_t)h + 1]; q += FE2_CHUNK) {
      pl.chunk_start.push_back(q);
      pl.chunk_level.push_back(h);
    }
  pl.chunk_start.push_back(n);
  // union-find over the G + H levels: a row links its two levels, whatever its weight
  std::vector<int32_t> par((size_t)G + (size_t)H);
  std::iota(par.begin(), par.end(), 0);
  auto find = [&par](int32_t x) {
    while (par[(size_t)x] != x) {
      par[(size_t)x] = par[(size_t)par[(size_t)x]];
      x = par[(size_t)x];
    }
    return x;
  };
  for (int64_t i = 0; i < n; ++i) {
    const int32_t a = find(ids1[i]), b = find(G + ids2[i]);
    if (a != b) par[(size_t)std::max(a, b)] = std::min(a, b);
  }
  pl.comp1.assign((size_t)G, -1);
  pl.comp2.assign((size_t)H, -1);
  pl.low.clear();
  pl.nlev2.clear();
  std::vector<int32_t> of_root((size_t)G + (size_t)H, -1);
  for (int32_t h = 0; h < H; ++h) {
    if (ptr[(size_t)h + 1] == ptr[(size_t)h]) continue;
    const int32_t r = find(G + h);
    if (of_root[(size_t)r] < 0) {
      of_root[(size_t)r] = (int32_t)pl.low.size();
      pl.low.push_back(h);
      pl.nlev2.push_back(0);
    }
    pl.comp2[(size_t)h] = of_root[(size_t)r];
    pl.nlev2[(size_t)of_root[(size_t)r]] += 1;
  }
  for (int64_t i = 0; i < n; ++i) pl.comp1[(size_t)ids1[i]] = of_root[(size_t)find(ids1[i])];
  return true;
}

double default_tol(const sglm_fe2_opts* o) { return o && o->sweep_tol > 0.0 ? o->sweep_tol : 1e-12; }
int default_sweeps(const sglm_fe2_opts* o) { return o && o->max_sweeps > 0 ? o->max_sweeps : 10000; }

}  // namespace

struct sglm_engine::Fe2State {
  int32_t H = 0, ncomp = 0;
  int64_t nchunk = 0, ld2 = 0, ldy = 0, prow = 0;
  bool all_pinned = false;  // every factor-2 level is alone in its component: c = 0, one sweep is exact
  int32_t *did1 = nullptr, *did2 = nullptr, *dpin = nullptr, *dcomp1 = nullptr, *dcomp2 = nullptr, *dlow = nullptr;
  // list [n] | chunk_start [nchunk + 1] | per combine level chunk_start [nchunk_l + 1], chunk_dst [nchunk_l] |
  // order [nchunk]: the chunks by their first row, the order in which the kernels' work units take them
  int64_t* didx = nullptr;
  int64_t n = 0, order_off = 0;
  const int64_t* list() const { return didx; }
  const int64_t* chunks() const { return didx + n; }
  const int64_t* order() const { return didx + order_off; }
  std::vector<sglm_engine::CombineLevel> levels;
  // allocated by prepare (they depend on p and on the cluster factor's buffers)
  int64_t ld1 = 0;
  double *dR2 = nullptr, *dP2 = nullptr, *dS2 = nullptr, *dT2 = nullptr, *dT1 = nullptr, *dRg = nullptr, *dPg = nullptr;
  double *dY1 = nullptr, *dY2 = nullptr, *dwz = nullptr, *dgamma = nullptr, *dgraw = nullptr;
  double *dcpart = nullptr, *dcross = nullptr;
  unsigned long long* dstop = nullptr;
  int64_t slice_rows[2] = {0, 0};
  int nslice[2] = {0, 0};
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

void sglm_engine::free_fe2() {
  if (!fe2) return;
  for (int32_t** q : {&fe2->did1, &fe2->did2, &fe2->dpin, &fe2->dcomp1, &fe2->dcomp2, &fe2->dlow}) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  if (fe2->didx) (void)hipFree(fe2->didx);
  if (fe2->dstop) (void)hipFree(fe2->dstop);
  dev_free({&fe2->dR2, &fe2->dP2, &fe2->dS2, &fe2->dT2, &fe2->dT1, &fe2->dRg, &fe2->dPg, &fe2->dY1, &fe2->dY2,
            &fe2->dwz, &fe2->dgamma, &fe2->dgraw, &fe2->dcpart, &fe2->dcross});
  for (hipEvent_t& e : fe2->ev)
    if (e) (void)hipEventDestroy(e);
  delete fe2;
  fe2 = nullptr;
}

namespace {

using Fe2 = sglm_engine::Fe2State;

template <class T>
int upload(T** dst, const std::vector<T>& v, const char* what) {
  const size_t bytes = sizeof(T) * std::max<size_t>(v.size(), 1);
  hipError_t e = hipMalloc((void**)dst, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(hip_msg(e, what));
    return SGLM_ENOMEM;
  }
  if (!v.empty()) HIPCHK(hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return SGLM_OK;
}

// the cluster factor's code of every resident row, from the segments the device keeps
int cluster_ids(sglm_engine* s, std::vector<int32_t>& ids1) {
  std::vector<int64_t> start((size_t)s->cl_nseg + 1), clus((size_t)std::max<int64_t>(s->cl_nseg, 1));
  HIPCHK(hipMemcpy(start.data(), s->seg_start(), sizeof(int64_t) * start.size(), hipMemcpyDeviceToHost));
  if (s->cl_nseg > 0)
    HIPCHK(hipMemcpy(clus.data(), s->seg_cluster(), sizeof(int64_t) * (size_t)s->cl_nseg,
                     hipMemcpyDeviceToHost));
  ids1.assign((size_t)s->n, 0);
  for (int64_t k = 0; k < s->cl_nseg; ++k)
    for (int64_t i = start[(size_t)k]; i < start[(size_t)k + 1]; ++i) ids1[(size_t)i] = (int32_t)clus[(size_t)k];
  return SGLM_OK;
}

// The second factor of this shard's rows: the lists, their chunks, the combine's levels over them, the components
int set_fe2_local(sglm_engine* s, const int32_t* ids2, int32_t H) {
  HIPCHK(hipSetDevice(s->device));
  s->free_fe2();
  std::vector<int32_t> ids1;
  if (int rc = cluster_ids(s, ids1)) return rc;
  Fe2Plan pl;
  if (!fe2_plan(ids1.data(), ids2, s->n, s->cl_G, H, pl)) {
    set_error("requirement failed: every code of the second factor in [0, H = " + std::to_string(H) + ")");
    return SGLM_EINVAL;
  }
  Fe2* F = s->fe2 = new Fe2();
  F->H = H;
  F->n = s->n;
  F->ncomp = (int32_t)pl.low.size();
  F->nchunk = (int64_t)pl.chunk_level.size();
  F->ld2 = ((int64_t)H + 31) / 32 * 32;
  F->ldy = (s->p + 1 + 7) / 8 * 8;
  std::vector<int32_t> pin((size_t)H, 0);
  F->all_pinned = true;
  for (int32_t h = 0; h < H; ++h) {
    const int32_t c = pl.comp2[(size_t)h];
    pin[(size_t)h] = c < 0 || pl.nlev2[(size_t)c] == 1 ? 1 : 0;
    F->all_pinned = F->all_pinned && pin[(size_t)h];
  }
  // the combine's levels over the chunks, which are ordered by level already (vcov_cluster.cpp's rule)
  std::vector<int64_t> idx(pl.list);
  idx.insert(idx.end(), pl.chunk_start.begin(), pl.chunk_start.end());
  std::vector<CombineRange> open;
  for (int64_t k = 0; k < F->nchunk; ++k) {
    const int32_t level = pl.chunk_level[(size_t)k];
    if (open.empty() || open.back().dst != level) open.push_back({level, k, k + 1});
    else open.back().hi = k + 1;
  }
  F->prow = plan_combine(std::move(open), idx, F->levels);
  F->order_off = (int64_t)idx.size();
  {
    std::vector<int64_t> order((size_t)F->nchunk);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&pl](int64_t a, int64_t b) {
      return pl.list[(size_t)pl.chunk_start[(size_t)a]] < pl.list[(size_t)pl.chunk_start[(size_t)b]];
    });
    idx.insert(idx.end(), order.begin(), order.end());
  }
  std::vector<int32_t> id2(ids2, ids2 + s->n);
  int rc = upload(&F->did1, ids1, "hipMalloc(factor-1 codes)");
  if (!rc) rc = upload(&F->did2, id2, "hipMalloc(factor-2 codes)");
  if (!rc) rc = upload(&F->dpin, pin, "hipMalloc(pinned levels)");
  if (!rc) rc = upload(&F->dcomp1, pl.comp1, "hipMalloc(components)");
  if (!rc) rc = upload(&F->dcomp2, pl.comp2, "hipMalloc(components)");
  if (!rc) rc = upload(&F->dlow, pl.low, "hipMalloc(components)");
  if (!rc) rc = upload(&F->didx, idx, "hipMalloc(factor-2 row lists)");
  if (rc) s->free_fe2();
  return rc;
}

// The buffers of a two-way step (kept until the second factor, the clusters or the data change)
int fe2_prepare(sglm_engine* s) {
  Fe2* F = s->fe2;
  HIPCHK(hipSetDevice(s->device));
  for (hipEvent_t& e : F->ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  if (F->dS2) return SGLM_OK;
  const size_t d = sizeof(double);
  const int64_t p = s->p, G = s->cl_G, H = F->H;
  F->ld1 = s->cl_inner->n_pad;
  auto zalloc = [&](double** q, int64_t len, const char* what) -> int {
    len = std::max<int64_t>(len, 1);
    if (int rc = sglm_engine::dev_alloc(q, d * (size_t)len, what)) return rc;
    HIPCHK(hipMemsetAsync(*q, 0, d * (size_t)len, s->st));
    return SGLM_OK;
  };
  const int64_t nti = (p + 15) / 16, ntj = (p + 16) / 16;
  for (int f = 0; f < 2; ++f) {
    const int64_t L = f ? H : G;
    F->slice_rows[f] = (std::max<int64_t>(1024, (L + 63) / 64) + 3) / 4 * 4;
    F->nslice[f] = (int)((L + F->slice_rows[f] - 1) / F->slice_rows[f]);
  }
  int rc = zalloc(&F->dR2, F->nchunk * (p + 2), "hipMalloc(factor-2 chunk sums)");
  if (!rc) rc = zalloc(&F->dP2, F->prow * (p + 2), "hipMalloc(factor-2 combine scratch)");
  if (!rc) rc = zalloc(&F->dT2, F->ld2 * (p + 1), "hipMalloc(factor-2 sweep sums)");
  if (!rc) rc = zalloc(&F->dT1, F->ld1 * (p + 1), "hipMalloc(factor-1 sweep sums)");
  if (!rc) rc = zalloc(&F->dRg, std::max(s->cl_nseg, F->nchunk) * (p + 1), "hipMalloc(sweep unit sums)");
  if (!rc) rc = zalloc(&F->dPg, std::max(s->cl_prow, F->prow) * (p + 1), "hipMalloc(sweep combine scratch)");
  if (!rc) rc = zalloc(&F->dY1, G * F->ldy, "hipMalloc(factor-1 level coefficients)");
  if (!rc) rc = zalloc(&F->dY2, H * F->ldy, "hipMalloc(factor-2 level coefficients)");
  if (!rc) rc = zalloc(&F->dwz, s->n_pad, "hipMalloc(working responses)");
  if (!rc) rc = zalloc(&F->dgamma, H, "hipMalloc(factor-2 effects)");
  if (!rc) rc = zalloc(&F->dgraw, H, "hipMalloc(factor-2 effects)");
  if (!rc) rc = zalloc(&F->dcpart, (int64_t)(F->nslice[0] + F->nslice[1]) * 256 * nti * ntj, "hipMalloc(cross partials)");
  if (!rc) rc = zalloc(&F->dcross, 256 * nti * ntj, "hipMalloc(cross product)");
  if (!rc) {
    double* q = nullptr;
    rc = zalloc(&q, 2 * F->ldy, "hipMalloc(stop rule)");
    F->dstop = reinterpret_cast<unsigned long long*>(q);
  }
  if (!rc) rc = zalloc(&F->dS2, F->ld2 * (p + 2), "hipMalloc(factor-2 sums)");  // last: marks the set complete
  if (rc) {
    sglm_engine::dev_free({&F->dR2, &F->dP2, &F->dT2, &F->dT1, &F->dRg, &F->dPg, &F->dY1, &F->dY2, &F->dwz,
                           &F->dgamma, &F->dgraw, &F->dcpart, &F->dcross, &F->dS2});
    if (F->dstop) (void)hipFree(F->dstop);
    F->dstop = nullptr;
    return rc;
  }
  HIPCHK(hipStreamSynchronize(s->st));
  return SGLM_OK;
}

// what every two-way entry point requires, before any launch
int fe2_check(sglm_engine* h, const sglm_glm_opts* opts, int32_t* G) {
  if (!opts || !family_link_valid(opts->family, opts->link)) {
    set_error("requirement failed: opts with a supported family/link");
    return SGLM_EINVAL;
  }
  if (int rc = check_handle(h)) return rc;
  if (h->group() || h->comm.kind != 0) {
    set_error("requirement failed: a two-way fixed-effects fit runs on one device without a communicator (a "
              "multi-device handle or a handle with a communicator would need an all-reduce per sweep)");
    return SGLM_EINVAL;
  }
  if (int rc = fe_check(h, opts, G)) return rc;
  if (!h->fe2) {
    set_error("requirement failed: the second factor of the resident rows (sglm_set_fe2; a call that replaces the "
              "data or the clusters drops it)");
    return SGLM_EINVAL;
  }
  return fe2_prepare(h);
}

// the sums over factor 2's lists of [v x | r0 | r1] (ncolx = p) or of [r0 | r1] alone (ncolx = 0) into S
int list_sums(sglm_engine* s, int ncolx, const double* v, const double* r0, const double* r1, double* S) {
  Fe2* F = s->fe2;
  Fe2ListSumArgs a{};
  a.X = s->dX;
  a.ld = s->n_pad;
  a.p = ncolx;
  a.v = v;
  a.r0 = r0;
  a.r1 = r1;
  a.list = F->list();
  a.chunk_start = F->chunks();
  a.nchunk = F->nchunk;
  a.R = F->dR2;
  a.order = F->order();
  HIPCHK(launch_fe2_list_sum(a, s->ncu, s->st));
  return combine_levels(s, F->levels, F->didx, nullptr, F->dR2, F->dP2, ncolx + 2, S, F->ld2);
}

// T1[g, :] = sum_{i in g} v_i Y2[h(i), :] over the cluster factor's segments
int gather1(sglm_engine* s, const double* v) {
  Fe2* F = s->fe2;
  Fe2GatherArgs a{};
  a.v = v;
  a.id = F->did2;
  a.src = F->dY2;
  a.lds = F->ldy;
  a.nc = (int)s->p + 1;
  a.list = nullptr;
  a.start = s->seg_start();
  a.nunit = s->cl_nseg;
  a.R = F->dRg;
  HIPCHK(launch_fe2_gather(a, s->ncu, s->st));
  return s->combine_clusters(F->dRg, F->dPg, (int)s->p + 1, F->dT1, F->ld1);
}

// T2[h, :] = sum_{i in h} v_i Y1[g(i), :] over factor 2's chunks
int gather2(sglm_engine* s, const double* v) {
  Fe2* F = s->fe2;
  Fe2GatherArgs a{};
  a.v = v;
  a.id = F->did1;
  a.src = F->dY1;
  a.lds = F->ldy;
  a.nc = (int)s->p + 1;
  a.list = F->list();
  a.start = F->chunks();
  a.nunit = F->nchunk;
  a.R = F->dRg;
  a.order = F->order();
  HIPCHK(launch_fe2_gather(a, s->ncu, s->st));
  return combine_levels(s, F->levels, F->didx, nullptr, F->dRg, F->dPg, (int)s->p + 1, F->dT2, F->ld2);
}

int update_levels(sglm_engine* s, int f) {
  Fe2* F = s->fe2;
  Fe2UpdateArgs u{};
  u.S = f ? F->dS2 : s->fe.g;
  u.T = f ? F->dT2 : F->dT1;
  u.ldS = f ? F->ld2 : F->ld1;
  u.L = f ? F->H : s->cl_G;
  u.p = (int)s->p;
  u.pin = f ? F->dpin : nullptr;
  u.Y = f ? F->dY2 : F->dY1;
  u.ldy = F->ldy;
  u.stop = F->dstop;
  HIPCHK(launch_fe2_update(u, s->st));
  return SGLM_OK;
}

// The sweeps from the Y on the device, at the w in domega and the sums in fe.g / dS2
int run_sweeps(sglm_engine* s, const sglm_fe2_opts* o, int iter, int* sweeps) {
  Fe2* F = s->fe2;
  const double tol = default_tol(o);
  const int maxs = default_sweeps(o);
  const int64_t pc = s->p + 1;
  std::vector<unsigned long long> stop((size_t)(2 * F->ldy));
  double change = std::numeric_limits<double>::infinity();
  int k = 0;
  while (true) {
    ++k;
    HIPCHK(hipMemsetAsync(F->dstop, 0, sizeof(unsigned long long) * stop.size(), s->st));
    if (int rc = gather1(s, s->domega)) return rc;
    if (int rc = update_levels(s, 0)) return rc;
    if (F->all_pinned) break;  // c = 0: the system is the one-way one and this sweep solved it
    if (int rc = gather2(s, s->domega)) return rc;
    if (int rc = update_levels(s, 1)) return rc;
    HIPCHK(hipMemcpyAsync(stop.data(), F->dstop, sizeof(unsigned long long) * stop.size(), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    change = 0.0;
    bool nan = false;
    for (int64_t j = 0; j < pc; ++j) {
      double dj, mj;
      std::memcpy(&dj, &stop[(size_t)j], sizeof(double));
      std::memcpy(&mj, &stop[(size_t)(F->ldy + j)], sizeof(double));
      const double cj = dj == 0.0 ? 0.0 : dj / mj;
      nan = nan || std::isnan(cj);
      if (cj > change) change = cj;
    }
    if (nan) change = std::numeric_limits<double>::quiet_NaN();
    if (change <= tol) break;
    if (!std::isfinite(change) || k >= maxs) {
      set_error("requirement failed: the fixed-effects sweeps of iteration " + std::to_string(iter) +
                " did not converge: after " + std::to_string(k) + " sweep(s) (max_sweeps " + std::to_string(maxs) +
                ") the largest column-wise relative change is " + std::to_string(change) + " (sweep_tol " +
                std::to_string(tol) + ")");
      return SGLM_EINVAL;
    }
  }
  *sweeps = k;
  return SGLM_OK;
}

int offsets(sglm_engine* s) {
  Fe2* F = s->fe2;
  HIPCHK(hipSetDevice(s->device));
  Fe2OffsetArgs a{};
  a.off = s->doff;
  a.alpha = s->dalpha;
  a.gamma = F->dgamma;
  a.id1 = F->did1;
  a.id2 = F->did2;
  a.n = s->n;
  a.ld = s->n_pad;
  a.out = s->dfo;
  HIPCHK(launch_fe2_offset(a, s->st));
  s->off_override = s->dfo;
  return SGLM_OK;
}

int absorbed2_error(int64_t j) {
  set_error("breeze.linalg.MatrixSingularException: column " + std::to_string(j) + " of X is absorbed by the two "
            "factors' fixed effects (an intercept, or a regressor that is a sum of a function of factor 1's levels "
            "and one of factor 2's)");
  return SGLM_ESINGULAR;
}

float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();
    return 0.f;
  }
  return ms;
}

// One step at the device's (alpha, gamma, Y): packed = lower tri A | b | the pass's scalars
int fe2_step(sglm_engine* h, const sglm_fe2_opts* o, int family, int link, int mode, const double* beta, double mu0,
             bool check_absorbed, int iter, double* packed, int* sweeps) {
  Fe2* F = h->fe2;
  const int64_t p = h->p;
  if (int rc = offsets(h)) return rc;
  if (int rc = h->pass(mode, beta, mu0, 0.0, family, link, packed)) return rc;
  // w in domega, w z in dwz, S1 | t1 | W1 in fe.g
  if (int rc = fe_group_sums(h, FE_WZ, mode, family, link, mu0, F->dwz)) return rc;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventRecord(F->ev[0], h->st));
  if (int rc = list_sums(h, (int)p, h->domega, F->dwz, h->domega, F->dS2)) return rc;
  HIPCHK(hipEventRecord(F->ev[1], h->st));
  HIPCHK(hipEventRecord(F->ev[2], h->st));
  if (int rc = run_sweeps(h, o, iter, sweeps)) return rc;
  HIPCHK(hipEventRecord(F->ev[3], h->st));
  HIPCHK(hipEventRecord(F->ev[4], h->st));
  Fe2CrossArgs c{};
  c.S[0] = h->fe.g;
  c.S[1] = F->dS2;
  c.ldS[0] = F->ld1;
  c.ldS[1] = F->ld2;
  c.Y[0] = F->dY1;
  c.Y[1] = F->dY2;
  c.L[0] = h->cl_G;
  c.L[1] = F->H;
  for (int f = 0; f < 2; ++f) {
    c.slice_rows[f] = F->slice_rows[f];
    c.nslice[f] = F->nslice[f];
  }
  c.p = (int)p;
  c.ldy = F->ldy;
  c.part = F->dcpart;
  HIPCHK(launch_fe2_cross(c, F->dcross, h->st));
  HIPCHK(hipEventRecord(F->ev[5], h->st));
  const int64_t PC = 16 * ((p + 16) / 16), PR = 16 * ((p + 15) / 16);
  std::vector<double> D((size_t)(PR * PC));
  HIPCHK(hipMemcpyAsync(D.data(), F->dcross, sizeof(double) * D.size(), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  h->fe2_ms[0] = h->fe.ms[0];
  h->fe2_ms[1] = h->fe.ms[1] + h->fe.ms[2];
  h->fe2_ms[2] = elapsed(F->ev[0], F->ev[1]);
  h->fe2_ms[3] = elapsed(F->ev[2], F->ev[3]);
  h->fe2_ms[4] = elapsed(F->ev[4], F->ev[5]);
  // the downdate, its X block symmetrised: A is exactly symmetric
  for (int64_t i = 0; i < p; ++i)
    for (int64_t j = 0; j <= i; ++j) {
      const double down = 0.5 * (D[(size_t)(i * PC + j)] + D[(size_t)(j * PC + i)]);
      const int64_t k = i * (i + 1) / 2 + j;
      if (i == j && check_absorbed && packed[k] > 0.0 && !(packed[k] - down > FE_ABSORBED_RATIO * packed[k]))
        return absorbed2_error(j);
      packed[k] -= down;
    }
  for (int64_t i = 0; i < p; ++i) packed[tri_count(p) + i] -= D[(size_t)(i * PC + p)];
  return SGLM_OK;
}

// alpha += a_z - a_X beta, gamma += c_z - c_X beta from the Y and the weights of the last step, then the
// per-component normalisation: gamma of a component's lowest factor-2 code is 0
int effects_step(sglm_engine* h, const double* beta) {
  Fe2* F = h->fe2;
  HIPCHK(hipSetDevice(h->device));
  const int64_t p = h->p;
  std::memcpy(h->hbeta, beta, sizeof(double) * p);
  HIPCHK(hipMemcpyAsync(h->dbeta, h->hbeta, sizeof(double) * p, hipMemcpyHostToDevice, h->st));
  for (int f = 0; f < 2; ++f) {
    Fe2EffectArgs a{};
    a.Y = f ? F->dY2 : F->dY1;
    a.ldy = F->ldy;
    a.L = f ? F->H : h->cl_G;
    a.p = (int)p;
    a.W = f ? F->dS2 + (p + 1) * F->ld2 : h->fe.g + (p + 1) * F->ld1;
    a.beta = h->dbeta;
    a.eff = f ? F->dgamma : h->dalpha;
    HIPCHK(launch_fe2_effect(a, h->st));
  }
  HIPCHK(hipMemcpyAsync(F->dgraw, F->dgamma, sizeof(double) * (size_t)F->H, hipMemcpyDeviceToDevice, h->st));
  Fe2NormArgs n{};
  n.alpha = h->dalpha;
  n.gamma = F->dgamma;
  n.gamma_raw = F->dgraw;
  n.comp1 = F->dcomp1;
  n.comp2 = F->dcomp2;
  n.low = F->dlow;
  n.G = h->cl_G;
  n.H = F->H;
  HIPCHK(launch_fe2_normalise(n, h->st));
  return SGLM_OK;
}

int zero_Y(sglm_engine* h) {
  Fe2* F = h->fe2;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemsetAsync(F->dY1, 0, sizeof(double) * (size_t)(h->cl_G * F->ldy), h->st));
  HIPCHK(hipMemsetAsync(F->dY2, 0, sizeof(double) * (size_t)(F->H * F->ldy), h->st));
  return SGLM_OK;
}

// W1, W2 of the last step: levels of positive weight; the effects (where given) of the others become NaN
int count_levels(sglm_engine* h, int32_t* geff, int32_t* heff, double* alpha = nullptr, double* gamma = nullptr) {
  Fe2* F = h->fe2;
  std::vector<double> W1((size_t)h->cl_G), W2((size_t)F->H);
  if (int rc = download_cols(h, h->fe.g, F->ld1, h->cl_G, h->p + 1, 1, W1.data())) return rc;
  if (int rc = download_cols(h, F->dS2, F->ld2, F->H, h->p + 1, 1, W2.data())) return rc;
  *geff = count_weighted(W1, alpha);
  *heff = count_weighted(W2, gamma);
  return SGLM_OK;
}

struct Fe2Backend : public StepBackend {
  const sglm_fe2_opts* o;
  int iter = 0, sweeps_last = 0;
  int64_t sweeps_total = 0;
  Fe2Backend(sglm_engine* handle, const sglm_fe2_opts* opts) : StepBackend(handle), o(opts) {}
  int pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override {
    (void)ybar;
    if (beta)
      if (int rc = effects_step(h, beta)) return rc;
    if (int rc = fe2_step(h, o, family, link, mode, beta, mu0, true, iter, packed, &sweeps_last)) return rc;
    sweeps_total += sweeps_last;
    iter += 1;
    return SGLM_OK;
  }
};

// Levels without a finite effect: the rows of positive prior weight all have y = 0 (or all y = m), either factor
int uninformative2(sglm_engine* h, int family, int link) {
  if (family != FAM_BINOMIAL && family != FAM_POISSON && family != FAM_NEGBIN) return SGLM_OK;
  Fe2* F = h->fe2;
  const int64_t p = h->p;
  for (int f = 0; f < 2; ++f) {
    const int64_t L = f ? F->H : h->cl_G;
    std::vector<double> ab((size_t)(2 * L));
    if (f == 0) {  // y and m - y (or 1) of every row into dwz and domega on the way
      if (int rc = fe_group_sums(h, FE_CHECK, MODE_IRLS, family, link, 0.0, F->dwz, h->domega)) return rc;
      if (int rc = download_cols(h, h->fe.g, F->ld1, L, p, 2, ab.data())) return rc;
    } else {
      HIPCHK(hipSetDevice(h->device));
      if (int rc = list_sums(h, 0, nullptr, F->dwz, h->domega, F->dT2)) return rc;  // (p + 1 >= 2 columns)
      HIPCHK(hipStreamSynchronize(h->st));
      if (int rc = download_cols(h, F->dT2, F->ld2, L, 0, 2, ab.data())) return rc;
    }
    const auto [count, first] = uninformative_levels(ab);
    if (count == 0) continue;
    set_error("requirement failed: " + std::to_string(count) + " level(s) of factor " + std::to_string(f + 1) +
              " have no finite fixed effect -- every row of positive prior weight has y = 0" +
              (family == FAM_BINOMIAL ? " or y = m" : "") + "; the first is level " + std::to_string(first) +
              " of factor " + std::to_string(f + 1) + " (drop their rows, as fixest does, and check again)");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

}  // namespace

extern "C" {

int sglm_fe2_plan(const int32_t* ids1, const int32_t* ids2, int64_t n, int32_t G, int32_t H, int64_t* chunk_len,
                  int64_t* nchunk, int64_t* chunk_start, int32_t* chunk_level, int64_t* list, int32_t* ncomp,
                  int32_t* comp_low) {
  if (n < 0 || G < 0 || H < 0 || (n > 0 && (!ids1 || !ids2))) {
    set_error("requirement failed: n >= 0, G >= 0, H >= 0, ids1 [n], ids2 [n]");
    return SGLM_EINVAL;
  }
  if (chunk_len) *chunk_len = FE2_CHUNK;
  Fe2Plan pl;
  if (!fe2_plan(ids1, ids2, n, G, H, pl)) {
    set_error("requirement failed: every code in [0, G = " + std::to_string(G) + ") and [0, H = " + std::to_string(H) + ")");
    return SGLM_EINVAL;
  }
  if (nchunk) *nchunk = (int64_t)pl.chunk_level.size();
  if (chunk_start) std::copy(pl.chunk_start.begin(), pl.chunk_start.end(), chunk_start);
  if (chunk_level) std::copy(pl.chunk_level.begin(), pl.chunk_level.end(), chunk_level);
  if (list) std::copy(pl.list.begin(), pl.list.end(), list);
  if (ncomp) *ncomp = (int32_t)pl.low.size();
  if (comp_low) std::copy(pl.low.begin(), pl.low.end(), comp_low);
  return SGLM_OK;
}

int sglm_set_fe2(sglm_engine* h, const int32_t* ids2, int64_t n_local, int32_t H) {
  if (int rc = check_handle(h)) return rc;
  if (!ids2) {  // clears
    for (sglm_engine* s : h->shards()) s->free_fe2();
    h->free_fe2();
    return SGLM_OK;
  }
  if (h->group() || h->comm.kind != 0) {
    set_error("requirement failed: a second fixed-effects factor is declared on one device without a communicator");
    return SGLM_EINVAL;
  }
  if (int rc = check_ready(h)) return rc;
  if (h->cl_G < 1) {
    set_error("requirement failed: the first factor of the resident rows before the second (sglm_set_clusters)");
    return SGLM_EINVAL;
  }
  if (H < 1 || n_local != h->n) {
    set_error("requirement failed: H >= 1 and n_local = the handle's " + std::to_string(h->n) + " resident rows (got " +
              std::to_string(n_local) + ")");
    return SGLM_EINVAL;
  }
  return set_fe2_local(h, ids2, H);
}

int sglm_fit_glm_fe2(sglm_engine* h, const sglm_glm_opts* opts, const sglm_fe2_opts* fe2, sglm_preglm* out,
                     double* alpha, double* gamma, sglm_fe2_info* info) {
  if (!out || !out->coefs || !out->std_err || !alpha || !gamma) {
    set_error("requirement failed: out, out->coefs, out->std_err, alpha, gamma");
    return SGLM_EINVAL;
  }
  int32_t G = 0;
  if (int rc = fe2_check(h, opts, &G)) return rc;
  Fe2* F = h->fe2;
  FeScope scope(h);
  if (int rc = h->set_effects(h->dalpha, nullptr, G)) return rc;
  if (int rc = h->set_effects(F->dgamma, nullptr, F->H)) return rc;
  if (int rc = zero_Y(h)) return rc;
  if (int rc = uninformative2(h, opts->family, opts->link)) return rc;
  Fe2Backend be(h, fe2);
  if (int rc = drive_step_fit(be, *opts, out)) return rc;
  // the effects of the last pass (at out->coefs) and the weights of that pass: a level without weight has none
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(alpha, h->dalpha, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(gamma, F->dgamma, sizeof(double) * (size_t)F->H, hipMemcpyDeviceToHost));
  int32_t geff = 0, heff = 0;
  if (int rc = count_levels(h, &geff, &heff, alpha, gamma)) return rc;
  if (info) {
    info->G_eff = geff;
    info->H_eff = heff;
    info->ncomp = F->ncomp;
    info->sweeps_last = be.sweeps_last;
    info->sweeps_total = be.sweeps_total;
    info->df_residual = out->nrow - (double)h->p - (double)(geff + heff - F->ncomp);
    info->weights_ms = h->fe2_ms[0];
    info->sum1_ms = h->fe2_ms[1];
    info->sum2_ms = h->fe2_ms[2];
    info->sweep_ms = h->fe2_ms[3];
    info->cross_ms = h->fe2_ms[4];
  }
  return SGLM_OK;
}

int sglm_fe2_pass(sglm_engine* h, const sglm_glm_opts* opts, const sglm_fe2_opts* fe2, const double* beta,
                  const double* alpha, const double* gamma, double* A, double* b, double* group1, double* group2,
                  double* Y, double* scalars, int* sweeps) {
  int32_t G = 0;
  if (int rc = fe2_check(h, opts, &G)) return rc;
  Fe2* F = h->fe2;
  FeScope scope(h);
  const int64_t p = h->p, H = F->H;
  double mu0;
  int mode;
  if (int rc = fe_step_mode(h, opts, beta, &mode, &mu0)) return rc;
  if (int rc = h->set_effects(h->dalpha, alpha, G)) return rc;
  if (int rc = h->set_effects(F->dgamma, gamma, H)) return rc;
  if (int rc = zero_Y(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p));
  int k = 0;
  if (int rc = fe2_step(h, fe2, opts->family, opts->link, mode, beta, mu0, false, 0, packed.data(), &k)) return rc;
  fe_unpack_step(packed.data(), p, A, b, scalars);
  if (sweeps) *sweeps = k;
  if (group1)
    if (int rc = download_cols(h, h->fe.g, F->ld1, G, 0, p + 2, group1)) return rc;
  if (group2)
    if (int rc = download_cols(h, F->dS2, F->ld2, H, 0, p + 2, group2)) return rc;
  if (Y) {
    HIPCHK(hipSetDevice(h->device));
    const int64_t L = (int64_t)G + H;
    std::vector<double> y1((size_t)(G * F->ldy)), y2((size_t)(H * F->ldy));
    HIPCHK(hipMemcpy(y1.data(), F->dY1, sizeof(double) * y1.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(y2.data(), F->dY2, sizeof(double) * y2.size(), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j <= p; ++j) {
      for (int64_t l = 0; l < G; ++l) Y[j * L + l] = y1[(size_t)(l * F->ldy + j)];
      for (int64_t l = 0; l < H; ++l) Y[j * L + G + l] = y2[(size_t)(l * F->ldy + j)];
    }
  }
  return SGLM_OK;
}

int sglm_vcov_fe2(sglm_engine* h, const sglm_glm_opts* opts, const sglm_fe2_opts* fe2, const double* beta,
                  const double* alpha, const double* gamma, int cluster, int hc_type, int cadjust, double* cov,
                  double* meat) {
  if (!beta || !alpha || !gamma || !cov) {
    set_error("requirement failed: beta, alpha, gamma, cov");
    return SGLM_EINVAL;
  }
  if (cluster)
    if (int rc = check_cluster_hc(hc_type)) return rc;
  int32_t G = 0;
  if (int rc = fe2_check(h, opts, &G)) return rc;
  if (cluster)
    if (int rc = check_cadjust(cadjust, G)) return rc;
  Fe2* F = h->fe2;
  FeScope scope(h);
  const int64_t p = h->p;
  if (int rc = h->set_effects(h->dalpha, alpha, G)) return rc;
  if (int rc = h->set_effects(F->dgamma, gamma, F->H)) return rc;
  if (int rc = zero_Y(h)) return rc;
  std::vector<double> packed((size_t)packed_len(p)), C((size_t)(p * p)), M((size_t)(p * p)), x((size_t)p);
  int k = 0;
  if (int rc = fe2_step(h, fe2, opts->family, opts->link, MODE_IRLS, beta, 0.0, true, 0, packed.data(), &k)) return rc;
  const char* singular = "breeze.linalg.MatrixSingularException: the two-way within X'WX is singular";
  if (int rc = bread(h, packed.data(), singular, C.data())) return rc;
  if (!cluster) return fe_plain_cov(C, cov, meat);
  int32_t geff = 0, heff = 0;
  if (int rc = count_levels(h, &geff, &heff)) return rc;
  // the u-weighted sums S | U over factor 1 into fe.g (u in domega), then sum_{i in g} u_i c_{h(i)} into T1
  if (int rc = fe_group_sums(h, FE_SCORE, MODE_IRLS, opts->family, opts->link, 0.0)) return rc;
  HIPCHK(hipSetDevice(h->device));
  if (int rc = gather1(h, h->domega)) return rc;
  sglm_engine* in = h->cl_inner;
  Fe2MeatArgs m{};
  m.Su = h->fe.g;
  m.Tu = F->dT1;
  m.Y1 = F->dY1;
  m.G = G;
  m.ld = in->n_pad;
  m.ldy = F->ldy;
  m.p = (int)p;
  m.X = in->dX;
  m.y = in->dy;
  HIPCHK(launch_fe2_meat(m, h->st));
  HIPCHK(hipStreamSynchronize(h->st));  // the internal engine's pass runs on its own stream
  h->cl_S_stale = true;                 // the cluster-robust covariance's S lives in the same design
  if (int rc = in->pass(MODE_LM_GRAM, nullptr, 0.0, 0.0, FAM_GAUSSIAN, LNK_IDENTITY, packed.data())) return rc;
  unpack_gram(packed.data(), p, M.data(), x.data());
  // nrows: every row, weight 0 included
  const int64_t absorbed = geff + heff - F->ncomp;
  return clustered_finish(hc_type, (double)h->n, p, absorbed, G, cadjust, C, M, "(beta, alpha, gamma)", cov, meat);
}

int sglm_get_fe2_ms(sglm_engine* h, double* ms) {
  if (int rc = check_handle(h)) return rc;
  if (!ms) {
    set_error("requirement failed: ms [5]");
    return SGLM_EINVAL;
  }
  for (int k = 0; k < 5; ++k) ms[k] = h->fe2_ms[k];
  return SGLM_OK;
}

}  // extern "C"
