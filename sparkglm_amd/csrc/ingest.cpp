// ingest.cpp -- data in and predictions out: pageable host rows through pinned staging into the
// resident shard (sglm_reserve / sglm_set_rows / sglm_set_data), device and synthetic shards,
// sglm_get_data, and the predictions of resident and new rows (sglm_predict*).
#include <algorithm>
#include <cstring>
#include <iterator>

#include "engine.hpp"

using namespace sglm;

// Copy a column-major host block (rows x cols, leading dimension sld) into a packed buffer,
// on several threads for large blocks (the pageable -> pinned leg of the ingest path).
static void pack_cols(double* dst, const double* src, int64_t sld, int64_t rows, int64_t cols) {
  const int64_t total = rows * cols;
  const int hw = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  const int nt = total >= ((int64_t)2 << 20) ? hw : 1;  // >= 16 MiB: split the copy
  auto part = [&](int t) {
    if (cols >= nt) {
      for (int64_t c = t; c < cols; c += nt) std::memcpy(dst + c * rows, src + c * sld, sizeof(double) * rows);
    } else {
      const int64_t r0 = rows * t / nt, r1 = rows * (t + 1) / nt;
      for (int64_t c = 0; c < cols; ++c)
        std::memcpy(dst + c * rows + r0, src + c * sld + r0, sizeof(double) * (size_t)(r1 - r0));
    }
  };
  if (nt == 1) {
    part(0);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(part, t);
  part(0);
  for (auto& x : th) x.join();
}

// ---- ingest: pageable host -> pinned staging -> HBM ----
int sglm_engine::ensure_staging() {
  if (hstage[0]) return SGLM_OK;
  for (int k = 0; k < 2; ++k) {
    HIPCHK(hipHostMalloc(&hstage[k], sizeof(double) * STAGE_DOUBLES, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&evstage[k], hipEventDisableTiming));
    HIPCHK(hipEventRecord(evstage[k], st));
  }
  return SGLM_OK;
}

// Column-major host block (rows x cols, leading dimension sld) -> device (leading dimension
// dld) through the two pinned buffers: the CPU packs one while the DMA engine drains the
// other.  Pageable memory is never handed to the DMA engine directly.
int sglm_engine::h2d_block(double* dst, int64_t dld, const double* src, int64_t sld, int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return SGLM_OK;
  int rc = ensure_staging();
  if (rc) return rc;
  const int64_t rchunk = std::min<int64_t>(rows, STAGE_DOUBLES);
  for (int64_t r0 = 0; r0 < rows; r0 += rchunk) {
    const int64_t rr = std::min(rchunk, rows - r0);
    const int64_t cchunk = std::max<int64_t>(1, STAGE_DOUBLES / rr);
    for (int64_t c0 = 0; c0 < cols; c0 += cchunk) {
      const int64_t cc = std::min(cchunk, cols - c0);
      const int k = stage_k;
      stage_k ^= 1;
      HIPCHK(hipEventSynchronize(evstage[k]));  // the copy that last read this buffer is done
      pack_cols(hstage[k], src + r0 + c0 * sld, sld, rr, cc);
      HIPCHK(hipMemcpy2DAsync(dst + r0 + c0 * dld, sizeof(double) * (size_t)dld, hstage[k], sizeof(double) * rr,
                              sizeof(double) * rr, (size_t)cc, hipMemcpyHostToDevice, st));
      HIPCHK(hipEventRecord(evstage[k], st));
    }
  }
  return SGLM_OK;
}

// Rows [row0, row0 + nr) of the reserved shard from host memory (sglm_set_rows).
int sglm_engine::set_rows(int64_t row0, int64_t nr, const double* X, int64_t ldx, const double* yv, const double* mv,
                          const double* ov, const double* pv) {
  HIPCHK(hipSetDevice(device));
  if (p <= 0 || procx.on) {
    set_error("requirement failed: sglm_reserve the shard before sglm_set_rows");
    return SGLM_EINVAL;
  }
  if (row0 < 0 || nr < 0 || row0 + nr > n || (nr > 0 && (!X || !yv || ldx < nr))) {
    set_error("requirement failed: 0 <= row0, row0 + nrows <= reserved rows, X and y non-null, ldx >= nrows");
    return SGLM_EINVAL;
  }
  if ((mv != nullptr) != (dm != nullptr) || (ov != nullptr) != (doff != nullptr) ||
      (pv != nullptr) != (dprior != nullptr)) {
    set_error("requirement failed: m / offset / prior must be given exactly when they were reserved");
    return SGLM_EINVAL;
  }
  if (nr == 0) return SGLM_OK;
  // blocks must not overlap (sglm.h): a repeated or overlapping block would count its rows twice
  // and let a fit run over reserved rows that were never written (zero X, y)
  auto it = std::lower_bound(written.begin(), written.end(), std::make_pair(row0, row0));
  if ((it != written.end() && it->first < row0 + nr) || (it != written.begin() && std::prev(it)->second > row0)) {
    set_error("requirement failed: rows [" + std::to_string(row0) + ", " + std::to_string(row0 + nr) +
              ") overlap a block already written (sglm_set_rows blocks must not overlap)");
    return SGLM_EINVAL;
  }
  const double t0 = now_ms();
  int rc = h2d_block(dX + row0, n_pad, X, ldx, nr, p);
  for (auto pr : {std::make_pair(dy, yv), std::make_pair(dm, mv), std::make_pair(doff, ov),
                  std::make_pair(dprior, pv)})
    if (!rc && pr.second) rc = h2d_block(pr.first + row0, n_pad, pr.second, nr, nr, 1);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st));
  load_ms += now_ms() - t0;
  const int nvec = 1 + (mv != nullptr) + (ov != nullptr) + (pv != nullptr);
  load_bytes += (int64_t)sizeof(double) * nr * (p + nvec);
  it = written.insert(std::lower_bound(written.begin(), written.end(), std::make_pair(row0, row0)),
                      std::make_pair(row0, row0 + nr));
  if (std::next(it) != written.end() && std::next(it)->first == it->second) {  // merge touching neighbours
    it->second = std::next(it)->second;
    written.erase(std::next(it));
  }
  if (it != written.begin() && std::prev(it)->second == it->first) {
    std::prev(it)->second = it->second;
    written.erase(it);
  }
  rows_loaded += nr;
  return SGLM_OK;
}

int sglm_engine::check_loaded() const {
  if (p <= 0) {
    set_error("requirement failed: no data set (sglm_set_data)");
    return SGLM_EINVAL;
  }
  if (!procx.on && rows_loaded < n) {
    set_error("requirement failed: " + std::to_string(n - rows_loaded) +
              " reserved rows were never written (sglm_set_rows)");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

// ---- scoring of new rows (sglm_predict_new, sglm_predict_new_se): its own scratch, the shard stays resident ----
// dxs holds chunk rows of pp columns; dvs / dms / dos chunk values each
int sglm_engine::ensure_new_rows(int64_t pp, int64_t chunk) {
  if (int rc = grow(dxs, xs_cap, pp * chunk, "hipMalloc(new rows)")) return rc;
  if (chunk > vs_cap) {
    vs_cap = 0;
    for (double** q : {&dvs, &dms, &dos}) {
      int64_t none = 0;
      if (int rc = grow(*q, none, chunk, "hipMalloc(new rows)")) return rc;
    }
    vs_cap = chunk;
  }
  return SGLM_OK;
}

int sglm_engine::predict_new(const double* X, int64_t nn, int64_t pp, int64_t ldx, const double* beta,
                             const double* off, const double* mv, int family, int link, int type, double* out) {
  HIPCHK(hipSetDevice(device));
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nn, ((int64_t)1 << 27) / std::max<int64_t>(pp, 1)));
  int rc = ensure_new_rows(pp, chunk);
  if (!rc) rc = ensure_red_len(pp);  // hbeta / dbeta (scoring before any shard exists)
  if (rc) return rc;
  std::memcpy(hbeta, beta, sizeof(double) * pp);
  HIPCHK(hipMemcpyAsync(dbeta, hbeta, sizeof(double) * pp, hipMemcpyHostToDevice, st));
  for (int64_t r0 = 0; r0 < nn; r0 += chunk) {
    const int64_t nr = std::min(chunk, nn - r0);
    rc = h2d_block(dxs, nr, X + r0, ldx, nr, pp);
    if (!rc && off) rc = h2d_block(dos, nr, off + r0, nr, nr, 1);
    if (!rc && mv) rc = h2d_block(dms, nr, mv + r0, nr, nr, 1);
    if (rc) return rc;
    HIPCHK(launch_predict(dxs, nr, (int)pp, nr, dbeta, off ? dos : nullptr, dvs, st, ProcX{}));
    if (type == SGLM_PREDICT_RESPONSE) HIPCHK(launch_unlink(dvs, mv ? dms : nullptr, nr, family, link, st));
    HIPCHK(hipMemcpyAsync(out + r0, dvs, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return SGLM_OK;
}

// Row ranges of a multi-device handle's shards: Spark's slicing [d n / D, (d+1) n / D).
static void group_split(sglm_engine* h, int64_t n) {
  const int64_t D = (int64_t)h->subs.size();
  h->sub_lo.assign((size_t)D + 1, 0);
  for (int64_t d = 0; d <= D; ++d) h->sub_lo[(size_t)d] = (int64_t)((__int128)d * n / D);
  h->g_n = n;
}

static int reserve_impl(sglm_engine* h, int64_t n, int64_t p, int has_m, int has_off, int has_prior) {
  h->consts_family = -1;
  if (n <= 0 || p <= 0) {
    set_error("requirement failed: n >= 1, p >= 1");
    return SGLM_EINVAL;
  }
  if (h->group()) {
    if (n < (int64_t)h->subs.size()) {
      set_error("requirement failed: at least one row per device");
      return SGLM_EINVAL;
    }
    group_split(h, n);
    for (size_t d = 0; d < h->subs.size(); ++d)
      if (int rc = reserve_impl(h->subs[d], h->sub_lo[d + 1] - h->sub_lo[d], p, has_m, has_off, has_prior)) return rc;
    return SGLM_OK;
  }
  return h->alloc_data(n, p, has_m != 0, has_off != 0, has_prior != 0);
}

static int set_rows_impl(sglm_engine* h, int64_t row0, int64_t nr, const double* X, int64_t ldx, const double* y,
                         const double* m, const double* off, const double* prior) {
  h->consts_family = -1;
  if (!h->group()) return h->set_rows(row0, nr, X, ldx, y, m, off, prior);
  if (h->g_n <= 0 || row0 < 0 || nr < 0 || row0 + nr > h->g_n) {
    set_error("requirement failed: sglm_reserve first; 0 <= row0, row0 + nrows <= reserved rows");
    return SGLM_EINVAL;
  }
  for (size_t d = 0; d < h->subs.size(); ++d) {  // the block's intersection with each shard
    const int64_t a = std::max(row0, h->sub_lo[d]), b = std::min(row0 + nr, h->sub_lo[d + 1]);
    if (a >= b) continue;
    const int64_t o = a - row0;
    auto sh = [&](const double* v) { return v ? v + o : nullptr; };
    if (int rc = h->subs[d]->set_rows(a - h->sub_lo[d], b - a, X + o, ldx, sh(y), sh(m), sh(off), sh(prior)))
      return rc;
  }
  return SGLM_OK;
}

static int synth_impl(sglm_engine* h, int kind, int64_t row0, int64_t n, int64_t p, uint64_t seed, bool proc) {
  h->consts_family = -1;
  if (kind < 0 || kind > 3 || n <= 0 || p <= 0 || row0 < 0) {
    set_error("requirement failed: synth kind in {0,1,2,3}, n >= 1, p >= 1");
    return SGLM_EINVAL;
  }
  if (h->group()) {
    if (n < (int64_t)h->subs.size()) {
      set_error("requirement failed: at least one row per device");
      return SGLM_EINVAL;
    }
    group_split(h, n);
    for (size_t d = 0; d < h->subs.size(); ++d)
      if (int rc = synth_impl(h->subs[d], kind, row0 + h->sub_lo[d], h->sub_lo[d + 1] - h->sub_lo[d], p, seed, proc))
        return rc;
    return SGLM_OK;
  }
  int rc = h->alloc_data(n, p, false, kind == 2, kind == 2, proc);
  if (rc) return rc;
  const double scale = 1.0 / std::sqrt((double)p);
  // procedural: y (and offset / prior) from the same generator; X itself is not stored
  HIPCHK(launch_synth(kind, row0, n, (int)p, seed, scale, proc ? nullptr : h->dX, h->n_pad, h->dy, nullptr, h->doff,
                      h->dprior, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  h->rows_loaded = n;
  h->written.assign(1, std::make_pair((int64_t)0, n));
  if (proc) {
    h->procx.on = 1;
    h->procx.kind = kind;
    h->procx.p = (int)p;
    h->procx.row0 = row0;
    h->procx.n = n;
    h->procx.kx = splitmix64_host(seed);
    h->procx.scale = scale;
    if (int rc2 = h->setup_proc_chunks()) return rc2;
  }
  return SGLM_OK;
}

static int get_data_impl(sglm_engine* h, double* X, int64_t ldx, double* y, double* m, double* offset,
                         double* prior) {
  if (h->group()) {
    for (size_t d = 0; d < h->subs.size(); ++d) {
      const int64_t o = h->sub_lo[d];
      auto sh = [&](double* v) { return v ? v + o : nullptr; };
      if (int rc = get_data_impl(h->subs[d], X ? X + o : nullptr, ldx, sh(y), sh(m), sh(offset), sh(prior)))
        return rc;
    }
    return SGLM_OK;
  }
  if (X && h->procx.on) {
    set_error("requirement failed: a procedural shard stores no X");
    return SGLM_EINVAL;
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t vb = sizeof(double) * (size_t)h->n;
  if (X)
    HIPCHK(hipMemcpy2DAsync(X, sizeof(double) * (size_t)ldx, h->dX, sizeof(double) * h->n_pad, vb, (size_t)h->p,
                            hipMemcpyDeviceToHost, h->st));
  if (y) HIPCHK(hipMemcpyAsync(y, h->dy, vb, hipMemcpyDeviceToHost, h->st));
  if (m && h->dm) HIPCHK(hipMemcpyAsync(m, h->dm, vb, hipMemcpyDeviceToHost, h->st));
  if (offset && h->doff) HIPCHK(hipMemcpyAsync(offset, h->doff, vb, hipMemcpyDeviceToHost, h->st));
  if (prior && h->dprior) HIPCHK(hipMemcpyAsync(prior, h->dprior, vb, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return SGLM_OK;
}

// eta (+ offset) of the resident rows -- or, type SGLM_PREDICT_RESPONSE, mu = unlink(eta, m) --
// into out [n_local]; a multi-device handle concatenates its shards in row order.
static int predict_resident(sglm_engine* h, const double* beta, int add_offset, int family, int link, int type,
                            double* out) {
  if (h->group()) {
    for (size_t d = 0; d < h->subs.size(); ++d)
      if (int rc = predict_resident(h->subs[d], beta, add_offset, family, link, type, out + h->sub_lo[d])) return rc;
    return SGLM_OK;
  }
  if (int rc = h->check_loaded()) return rc;
  HIPCHK(hipSetDevice(h->device));
  std::memcpy(h->hbeta, beta, sizeof(double) * h->p);
  HIPCHK(hipMemcpyAsync(h->dbeta, h->hbeta, sizeof(double) * h->p, hipMemcpyHostToDevice, h->st));
  HIPCHK(launch_predict(h->dX, h->n_pad, (int)h->p, h->n, h->dbeta, add_offset ? h->doff : nullptr, h->deta, h->st,
                        h->procx));
  if (type == SGLM_PREDICT_RESPONSE) HIPCHK(launch_unlink(h->deta, h->dm, h->n, family, link, h->st));
  HIPCHK(hipMemcpyAsync(out, h->deta, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return SGLM_OK;
}

extern "C" {

int sglm_reserve(sglm_engine* h, int64_t n, int64_t p, int has_m, int has_offset, int has_prior) {
  if (int rc = check_handle(h)) return rc;
  return reserve_impl(h, n, p, has_m, has_offset, has_prior);
}

int sglm_set_rows(sglm_engine* h, int64_t row0, int64_t nrows, const double* X, int64_t ldx, const double* y,
                  const double* m, const double* offset, const double* prior) {
  if (int rc = check_handle(h)) return rc;
  return set_rows_impl(h, row0, nrows, X, ldx, y, m, offset, prior);
}

int sglm_set_data(sglm_engine* h, const double* X, int64_t n, int64_t p, int64_t ldx, const double* y,
                  const double* m, const double* offset, const double* prior) {
  if (int rc = check_handle(h)) return rc;
  if (!X || !y || ldx < n || n <= 0 || p <= 0) {
    set_error("requirement failed: X, y non-null, n >= 1, p >= 1, ldx >= n");
    return SGLM_EINVAL;
  }
  int rc = reserve_impl(h, n, p, m != nullptr, offset != nullptr, prior != nullptr);
  if (rc) return rc;
  return set_rows_impl(h, 0, n, X, ldx, y, m, offset, prior);
}

int sglm_set_data_device(sglm_engine* h, const double* dX, int64_t n, int64_t p, int64_t ldx, const double* dy,
                         const double* dm, const double* doffset, const double* dprior) {
  if (int rc = check_handle(h)) return rc;
  if (h->group()) {
    set_error("requirement failed: sglm_set_data_device takes one device's memory; use a single-device handle");
    return SGLM_EINVAL;
  }
  if (!dX || !dy || ldx < n || n <= 0 || p <= 0) {
    set_error("requirement failed: X, y non-null, n >= 1, p >= 1, ldx >= n");
    return SGLM_EINVAL;
  }
  int rc = h->alloc_data(n, p, dm != nullptr, doffset != nullptr, dprior != nullptr);
  if (rc) return rc;
  const size_t vb = sizeof(double) * (size_t)n;
  const hipMemcpyKind kind = hipMemcpyDeviceToDevice;
  HIPCHK(hipMemcpy2DAsync(h->dX, sizeof(double) * h->n_pad, dX, sizeof(double) * ldx, vb, (size_t)p, kind, h->st));
  HIPCHK(hipMemcpyAsync(h->dy, dy, vb, kind, h->st));
  if (dm) HIPCHK(hipMemcpyAsync(h->dm, dm, vb, kind, h->st));
  if (doffset) HIPCHK(hipMemcpyAsync(h->doff, doffset, vb, kind, h->st));
  if (dprior) HIPCHK(hipMemcpyAsync(h->dprior, dprior, vb, kind, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  h->rows_loaded = n;
  h->written.assign(1, std::make_pair((int64_t)0, n));
  return SGLM_OK;
}

int sglm_synth(sglm_engine* h, int kind, int64_t row0, int64_t n, int64_t p, uint64_t seed) {
  if (int rc = check_handle(h)) return rc;
  return synth_impl(h, kind, row0, n, p, seed, false);
}

int sglm_synth_procedural(sglm_engine* h, int kind, int64_t row0, int64_t n, int64_t p, uint64_t seed) {
  if (int rc = check_handle(h)) return rc;
  return synth_impl(h, kind, row0, n, p, seed, true);
}

int sglm_get_data(sglm_engine* h, double* X, double* y, double* m, double* offset, double* prior) {
  if (int rc = check_handle(h)) return rc;
  return get_data_impl(h, X, h->group() ? h->g_n : h->n, y, m, offset, prior);
}

int sglm_predict(sglm_engine* h, const double* beta, int add_offset, double* out) {
  if (int rc = check_handle(h)) return rc;
  if (!beta || !out) {
    set_error("requirement failed: beta, out");
    return SGLM_EINVAL;
  }
  return predict_resident(h, beta, add_offset, FAM_GAUSSIAN, LNK_IDENTITY, SGLM_PREDICT_LINK, out);
}

int sglm_predict_glm(sglm_engine* h, const double* beta, int family, int link, int type, int add_offset,
                     double* out) {
  if (int rc = check_handle(h)) return rc;
  if (!beta || !out || !family_link_valid(family, link) || (type != SGLM_PREDICT_LINK && type != SGLM_PREDICT_RESPONSE)) {
    set_error("requirement failed: beta, out, a supported family/link, type link or response");
    return SGLM_EINVAL;
  }
  return predict_resident(h, beta, add_offset, family, link, type, out);
}

int sglm_predict_new(sglm_engine* h, const double* X, int64_t n, int64_t p, int64_t ldx, const double* beta,
                     const double* offset, const double* m, int family, int link, int type, double* out) {
  if (int rc = check_handle(h)) return rc;
  if (!X || !beta || !out || n < 0 || p <= 0 || ldx < n || !family_link_valid(family, link) ||
      (type != SGLM_PREDICT_LINK && type != SGLM_PREDICT_RESPONSE)) {
    set_error("requirement failed: X, beta, out, n >= 0, p >= 1, ldx >= n, a supported family/link, type link "
              "or response");
    return SGLM_EINVAL;
  }
  if (n == 0) return SGLM_OK;
  // new rows are scored on the first device
  return h->shards()[0]->predict_new(X, n, p, ldx, beta, offset, m, family, link, type, out);
}

}  // extern "C"
