// wide_path.cpp -- the engine's wide path (p > 256, SGLM_FORCE_WIDE=1, procedural shards): the
// Gram schedules and workspace of wide.hip's kernels, the wide pass in its three shapes
// (enqueue_wide), its timing, and the rocSOLVER device solver of the p x p system.
#include <rocsolver/rocsolver.h>

#include <algorithm>

#include "engine.hpp"
#include "solve.hpp"

using namespace sglm;

void sglm_engine::free_schedule() {
  for (int k = 0; k < 2; ++k) {
    if (dpieces[k]) (void)hipFree(dpieces[k]);
    if (dwgb[k]) (void)hipFree(dwgb[k]);
    dpieces[k] = nullptr;
    dwgb[k] = nullptr;
    has_sched[k] = false;
  }
  if (dstr) (void)hipFree(dstr);
  dstr = nullptr;
}

// Cost-balanced static schedules of the persistent Gram kernels.  For each kernel (off-
// diagonal / diagonal super-tiles) the (super-tile, block) line, super-tile major, is cut
// into ggrid equal segments; a segment's runs inside one super-tile are its pieces.
// Pieces are numbered in line order, so the partial slots of a super-tile are consecutive.
//
// Banded schedule: the k = ggrid / S workgroups of each of the S super-tiles take
// its blocks round-robin (block stride k), so all S k workgroups sweep the rows together and a
// block read by one super-tile's workgroup is read by the others' while it is still in the
// Infinity Cache / L2 (the workgroups that read the same blocks are numbered onto the same XCD,
// blockIdx % 8).  The E = ggrid - S k workgroups left over take the rows' tail, a fraction
// E / ggrid of every super-tile's blocks cut into E equal contiguous segments, so no workgroup
// idles and each carries the same work.  Slots of a super-tile: its k strided pieces, then its
// tail pieces in row order (the fixed reduction order).
// (shards too short to give every super-tile two workgroups keep the contiguous pieces)
bool sglm_engine::banded_kind(int S, int64_t nb, int G) const { return S > 0 && G / S >= 2 && nb >= 2; }

int sglm_engine::build_wide_schedule() {
  const int64_t nb = (nch > 0 ? ch_rows : nov > 0 ? ov_rows : n_pad) / WIDE_RB;
  std::vector<int> str((size_t)nst * 2, 0);
  free_schedule();
  int slot = 0;
  for (int kind = 0; kind < 2; ++kind) {
    std::vector<int> sts;
    for (int I = 0; I < npan; ++I)
      for (int J = 0; J <= I; ++J)
        if ((I == J) == (kind == 1)) sts.push_back(I * (I + 1) / 2 + J);
    if (sts.empty()) continue;
    const int G = ggk[kind];
    const int64_t total = nb * (int64_t)sts.size();
    std::vector<WidePiece> pieces;
    std::vector<int> wgb((size_t)G + 1, 0);
    if (banded_kind((int)sts.size(), nb, G)) {
      const int S = (int)sts.size();
      const int k = G / S, E = G - S * k;
      const int64_t tail = nb * E / G, nbm = nb - tail;  // banded blocks [0, nbm), tail [nbm, nb)
      const int per_xcd = std::max(1, G / 8);
      std::vector<int> gq((size_t)S * k), extra;  // pair q = j S + s -> workgroup; the left-over workgroups
      std::vector<char> used((size_t)G, 0);
      for (int q = 0; q < S * k; ++q) {
        const int g = (G % 8 == 0) ? (q % per_xcd) * 8 + q / per_xcd : q;
        gq[(size_t)q] = g;
        used[(size_t)g] = 1;
      }
      for (int g = 0; g < G; ++g)
        if (!used[(size_t)g]) extra.push_back(g);
      struct Pc { int g; int64_t b0, b1, bs; };
      std::vector<std::vector<Pc>> per_st((size_t)S);
      for (int j = 0; j < k; ++j)
        for (int s2 = 0; s2 < S; ++s2)
          if (j < nbm) per_st[(size_t)s2].push_back(Pc{gq[(size_t)j * S + s2], j, nbm, k});
      const int64_t tl = (int64_t)S * tail;  // tail line, super-tile major
      for (int e = 0; e < E && tl > 0; ++e) {
        int64_t pos = tl * e / E;
        const int64_t end = tl * (e + 1) / E;
        while (pos < end) {
          const int s2 = (int)(pos / tail);
          const int64_t b = pos % tail, len = std::min(tail - b, end - pos);
          per_st[(size_t)s2].push_back(Pc{extra[(size_t)e], nbm + b, nbm + b + len, 1});
          pos += len;
        }
      }
      std::vector<std::vector<WidePiece>> per_g((size_t)G);
      for (int s2 = 0; s2 < S; ++s2) {
        const int st = sts[(size_t)s2];
        str[(size_t)st * 2] = slot;
        for (const Pc& c : per_st[(size_t)s2]) per_g[(size_t)c.g].push_back(WidePiece{c.b0, c.b1, st, slot++, c.bs});
        str[(size_t)st * 2 + 1] = slot;
      }
      for (int g = 0; g < G; ++g) {
        wgb[(size_t)g] = (int)pieces.size();
        for (const WidePiece& w : per_g[(size_t)g]) pieces.push_back(w);
      }
      wgb[(size_t)G] = (int)pieces.size();
    } else {
      int64_t pos = 0, b = 0;
      size_t si = 0;
      for (int g = 0; g < G; ++g) {
        wgb[(size_t)g] = (int)pieces.size();
        const int64_t end = (int64_t)((__int128)total * (g + 1) / G);
        while (si < sts.size() && pos < end) {
          const int64_t k = std::min(nb - b, end - pos);
          const int st = sts[si];
          if (b == 0) str[(size_t)st * 2] = slot;
          pieces.push_back(WidePiece{b, b + k, st, slot++, 1});
          str[(size_t)st * 2 + 1] = slot;
          pos += k;
          b += k;
          if (b == nb) {
            ++si;
            b = 0;
          }
        }
      }
      wgb[(size_t)G] = (int)pieces.size();
    }
    HIPCHK(hipMalloc(&dpieces[kind], sizeof(WidePiece) * pieces.size()));
    HIPCHK(hipMalloc(&dwgb[kind], sizeof(int) * wgb.size()));
    HIPCHK(hipMemcpy(dpieces[kind], pieces.data(), sizeof(WidePiece) * pieces.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dwgb[kind], wgb.data(), sizeof(int) * wgb.size(), hipMemcpyHostToDevice));
    has_sched[kind] = true;
  }
  nslots = slot;
  HIPCHK(hipMalloc(&dstr, sizeof(int) * str.size()));
  HIPCHK(hipMemcpy(dstr, str.data(), sizeof(int) * str.size(), hipMemcpyHostToDevice));
  return SGLM_OK;
}

double* sglm_engine::rowpart(int c) const {
  return drp + (c == 0 ? 0 : ((int64_t)rgrid + (int64_t)(c - 1) * rgrid_ov) * NS);
}

// the events of a pass in nc chunks (evchunk)
int sglm_engine::ensure_chunk_events(int nc) {
  while (evchunk.size() < (size_t)4 * nc + 1) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    evchunk.push_back(e);
  }
  return SGLM_OK;
}

int sglm_engine::ensure_wide_workspace() {
  npan = wide_panels((int)p);
  nst = npan * (npan + 1) / 2;
  wstride = wide_stride();
  ggk[0] = ncu * wide_gram_wg_per_cu(false);
  ggk[1] = ncu * wide_gram_wg_per_cu(true);
  ggrid = ggk[0];
  nov = 0;
  ov_rows = 0;
  if (!procx.on && dX && ov_want > 1 && n_pad >= 2 * ov_min) {
    ov_rows = (std::max<int64_t>(ov_min, (n_pad + ov_want - 1) / ov_want) + 31) / 32 * 32;
    nov = (int)((n_pad + ov_rows - 1) / ov_rows);
    if (nov < 2) nov = 0, ov_rows = 0;
  }
  if (nov > 1) {
    if (!st2) HIPCHK(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
    if (int rc = ensure_chunk_events(nov)) return rc;
    if (dchunks) HIPCHK(hipFree(dchunks));
    dchunks = nullptr;
    HIPCHK(hipMalloc(&dchunks, sizeof(double) * (size_t)nov * (size_t)packed_len(p)));
  }
  int rc = build_wide_schedule();
  if (rc) return rc;
  grid = nslots;
  rgrid = (int)std::max<int64_t>(1, std::min<int64_t>(8 * (int64_t)ncu, ((nov > 0 ? ov_rows : n_pad) + 255) / 256));
  rgrid_ov = std::min(rgrid, ncu);
  if ((rc = grow(dgp, gp_cap, (int64_t)std::max(nslots, 1) * wstride, "hipMalloc(Gram partials)"))) return rc;
  // overlapped passes keep every chunk's row partials until its reduce (the next chunk's row
  // kernel runs meanwhile): chunk 0 at [0, rgrid), chunk c >= 1 at rgrid + (c - 1) rgrid_ov
  const int64_t need_rp = ((int64_t)rgrid + (int64_t)(std::max(ov_chunks(), 1) - 1) * rgrid_ov) * NS;
  if ((rc = grow(drp, rp_cap, need_rp, "hipMalloc(row partials)"))) return rc;
  if (!evm) HIPCHK(hipEventCreate(&evm));
  return SGLM_OK;
}

// Chunked procedural passes: the largest chunk the free HBM holds (minus a margin), balanced
// over the chunks; w / w*z cover nch * ch_rows rows (zero past n_pad).  Called once procx is set.
int sglm_engine::setup_proc_chunks() {
  if (!procx.on || !allow_chunks) return SGLM_OK;
  size_t fr = 0, tot = 0;
  HIPCHK(hipMemGetInfo(&fr, &tot));
  const int64_t ncols8 = (p + 7) / 8 * 8;
  const size_t margin = (size_t)4 << 30;
  size_t room = fr > margin ? fr - margin : 0;
  if (proc_scratch_max > 0) room = std::min(room, (size_t)proc_scratch_max << 30);
  const int64_t cap_rows = (int64_t)(room / (sizeof(double) * (size_t)ncols8));
  int64_t c = std::min<int64_t>(n_pad, cap_rows / 32 * 32);
  if (c < std::min<int64_t>(n_pad, (int64_t)1 << 20)) return SGLM_OK;  // too little room: in-kernel generation
  int64_t k = (n_pad + c - 1) / c;
  // overlapped: two scratch buffers, the row kernel of chunk c + 1 generates into one while the
  // Gram kernels of chunk c read the other; at least proc_ov_want chunks of >= 1M rows
  const int64_t half = cap_rows / 2 / 32 * 32, kmin = proc_ov_min;
  proc_ov = false;
  if (proc_ov_want > 1 && half >= kmin && n_pad >= 2 * kmin) {
    k = std::max<int64_t>((n_pad + half - 1) / half, std::min<int64_t>(proc_ov_want, n_pad / kmin));
    proc_ov = k >= 2;
  }
  c = ((n_pad + k - 1) / k + 31) / 32 * 32;
  ch_rows = c;
  nch = (int)((n_pad + c - 1) / c);
  const size_t sc = sizeof(double) * (size_t)c * (size_t)ncols8 * (proc_ov ? 2 : 1);
  HIPCHK(hipMalloc(&dxsc, sc));
  HIPCHK(hipMemsetAsync(dxsc, 0, sc, st));
  if (proc_ov && !st2) HIPCHK(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
  const int64_t span = (int64_t)nch * c;  // w / w*z rows the chunks address
  if (span > n_pad) {
    for (double** q : {&dw, &dwz}) {
      if (*q) HIPCHK(hipFree(*q));
      *q = nullptr;
      HIPCHK(hipMalloc(q, sizeof(double) * (size_t)span));
      HIPCHK(hipMemsetAsync(*q, 0, sizeof(double) * (size_t)span, st));
    }
  }
  HIPCHK(hipMalloc(&dchunks, sizeof(double) * (size_t)nch * (size_t)packed_len(p)));
  if (int rc = ensure_chunk_events(nch)) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return ensure_wide_workspace();  // the Gram schedule for ch_rows-row chunks
}

// The Gram kernels of one pass or chunk on st: the off-diagonal super-tiles' launch, then the
// diagonal ones' -- diag_first: the other way round.  None in a deviance-only pass.
int sglm_engine::launch_grams(WideGramArgs& g, bool diag_first) {
  for (int q = 0; q < 2 && !dev_only; ++q) {
    const int kind = diag_first ? 1 - q : q;
    if (!has_sched[kind]) continue;
    g.pieces = dpieces[kind];
    g.wg_begin = dwgb[kind];
    HIPCHK(launch_wide_gram(g, kind == 1, ggk[kind], st));
  }
  return SGLM_OK;
}

// The wide pass (enqueue_pass, wide): row stage -> Gram -> reduce into dred, in one of three shapes.
//   unchunked                 rows, Gram and reduce over the whole shard on st;
//   resident, nov chunks      every chunk's row kernel on st2, enqueued first; then per chunk on st:
//                             wait for its rows, Gram, reduce into dchunks[c];
//   procedural, nch chunks    per chunk: generate X into the scratch with the row stage (on st2 when
//                             overlapped, into the buffer chunk c - 2 has left; on st otherwise), then
//                             on st the Gram over the scratch, the diagonal launch first when
//                             overlapped, and the reduce into dchunks[c].
// The chunked shapes end with the ordered sum of dchunks into dred.
int sglm_engine::enqueue_wide(int mode, bool has_beta, double mu0, double ybar, int family, int link) {
  HIPCHK(hipEventRecord(ev0, st));
  WideRowArgs r{};
  r.X = dX;
  r.ld = n_pad;
  r.p = (int)p;
  r.y = dy;
  r.m = dm;
  r.off = doff;
  r.prior = dprior;
  r.beta = has_beta ? dbeta : nullptr;
  r.n = n;
  r.n_pad = n_pad;
  r.family = family;
  r.link = link;
  r.mode = mode;
  r.mu0 = mu0;
  r.ybar = ybar;
  r.theta = theta;
  r.w = dw;
  r.wz = dwz;
  r.eta_out = (mode == MODE_IRLS) ? deta : nullptr;
  r.row_partials = drp;
  r.proc = procx;
  r.r_begin = 0;
  r.r_end = n_pad;
  WideGramArgs g{};
  g.X = dX;
  g.ld = n_pad;
  g.ncols = (int)((p + 7) / 8 * 8);
  g.w = dw;
  g.wz = dwz;
  g.partials = dgp;
  g.stride = wstride;
  g.proc = procx;
  g.nb_lim = INT64_MAX;
  const int nc = chunks();
  if (nc == 0) {
    HIPCHK(launch_wide_rows(r, rgrid, st));
    HIPCHK(hipEventRecord(evm, st));
    if (int rc = launch_grams(g, false)) return rc;
    HIPCHK(hipEventRecord(ev1, st));
    HIPCHK(launch_wide_reduce(dgp, wstride, dstr, (int)p, drp, rgrid, dred, st));
    HIPCHK(hipEventRecord(ev2, st));
    return SGLM_OK;
  }
  const int64_t plen = packed_len(p);
  const bool fork = nov > 0 || proc_ov;  // the row kernels run on st2, beside the Gram on st
  const hipStream_t rs = fork ? st2 : st;
  const hipEvent_t* ev = evchunk.data();
  // chunk c's row kernel: the first on the whole-device grid, the others (beside a Gram) one workgroup per CU
  auto row_grid = [&](int c) { return fork && c > 0 ? rgrid_ov : rgrid; };
  auto row_part = [&](int c) { return fork ? rowpart(c) : drp; };
  // chunk c's Gram half on st, once its rows are done: Gram kernels over g, reduce into dchunks[c]
  auto gram_chunk = [&](int c) -> int {
    if (fork) HIPCHK(hipStreamWaitEvent(st, ev[4 * c + 1], 0));
    HIPCHK(hipEventRecord(ev[4 * c + 2], st));
    if (int rc = launch_grams(g, proc_ov)) return rc;  // procedural overlapped: the diagonal launch first
    HIPCHK(hipEventRecord(ev[4 * c + 3], st));
    HIPCHK(launch_wide_reduce(dgp, wstride, dstr, (int)p, row_part(c), row_grid(c), dchunks + (int64_t)c * plen, st));
    return SGLM_OK;
  };
  if (fork) {
    HIPCHK(hipEventRecord(ev[4 * nc], st));  // fork: beta uploaded, the last pass done
    HIPCHK(hipStreamWaitEvent(st2, ev[4 * nc], 0));
  }
  if (nch > 0) {  // procedural shard in chunks: generate C rows into the scratch, resident Gram over it
    const int64_t bufd = ch_rows * (int64_t)g.ncols;  // doubles per scratch buffer
    g.ld = ch_rows;
    g.proc = ProcX{};
    r.xs_ld = ch_rows;
    for (int c = 0; c < nch; ++c) {
      double* xs = dxsc + (proc_ov ? (int64_t)(c & 1) * bufd : 0);
      r.r_begin = (int64_t)c * ch_rows;
      r.r_end = r.r_begin + ch_rows;
      r.xs_out = dev_only ? nullptr : xs;  // deviance only: eta from the generator, no scratch
      r.row_partials = row_part(c);
      // buffer c & 1 is free once the Gram kernels of chunk c - 2 are done with it: chunk c's
      // generator then starts beside chunk c - 1's diagonal launch (which goes first, launch_grams)
      if (proc_ov && c >= 2) HIPCHK(hipStreamWaitEvent(st2, ev[4 * (c - 2) + 3], 0));
      HIPCHK(hipEventRecord(ev[4 * c], rs));
      if (!dev_only && proc_ov && c > 0) {
        // the lean generator (X into the scratch, X beta into deta), then the family stage from deta
        ProcGenArgs pg{};
        pg.proc = procx;
        pg.beta = mode == MODE_IRLS ? r.beta : nullptr;
        pg.xs = xs;
        pg.xs_ld = ch_rows;
        pg.r_begin = r.r_begin;
        pg.r_end = r.r_end;
        pg.eta_raw = deta;
        HIPCHK(launch_proc_gen(pg, 2 * ncu, rs));
        WideRowArgs rf = r;
        rf.xs_out = nullptr;
        rf.proc = ProcX{};
        rf.eta_in = mode == MODE_IRLS ? deta : nullptr;
        HIPCHK(launch_wide_rows(rf, rgrid_ov, rs, true));
      } else {
        HIPCHK(launch_wide_rows(r, row_grid(c), rs, proc_ov && c > 0));
      }
      HIPCHK(hipEventRecord(ev[4 * c + 1], rs));
      g.X = xs;
      g.w = dw + r.r_begin;
      g.wz = dwz + r.r_begin;
      if (int rc = gram_chunk(c)) return rc;
    }
    HIPCHK(hipEventRecord(evm, st));  // unused in chunked timing (wide_timing sums the chunks' spans)
  } else {  // resident: all row kernels on st2 first, then chunk c's Gram on st once its rows are done
    for (int c = 0; c < nov; ++c) {
      r.r_begin = (int64_t)c * ov_rows;
      r.r_end = std::min<int64_t>(n_pad, r.r_begin + ov_rows);
      r.row_partials = rowpart(c);
      HIPCHK(hipEventRecord(ev[4 * c], st2));
      HIPCHK(launch_wide_rows(r, row_grid(c), st2, c > 0));
      HIPCHK(hipEventRecord(ev[4 * c + 1], st2));
    }
    for (int c = 0; c < nov; ++c) {
      const int64_t r0 = (int64_t)c * ov_rows, r1 = std::min<int64_t>(n_pad, r0 + ov_rows);
      g.X = dX + r0;
      g.w = dw + r0;
      g.wz = dwz + r0;
      g.nb_lim = (r1 - r0) / WIDE_RB;
      if (int rc = gram_chunk(c)) return rc;
    }
  }
  HIPCHK(hipEventRecord(ev1, st));
  HIPCHK(launch_sum_chunks(dchunks, nc, (int)p, dred, st));
  HIPCHK(hipEventRecord(ev2, st));
  return SGLM_OK;
}

// Row-stage and Gram kernel times of the wide pass just synchronised (pass_timing; k1 = ev0 -> ev1).
int sglm_engine::wide_timing(float k1) {
  float km = 0.f, kg = 0.f;
  if (chunks() > 0) {  // chunked pass: row spans and Gram spans per chunk
    for (int c = 0; c < chunks(); ++c) {
      float kr = 0.f, kc = 0.f;
      HIPCHK(hipEventElapsedTime(&kr, evchunk[(size_t)4 * c], evchunk[(size_t)4 * c + 1]));
      HIPCHK(hipEventElapsedTime(&kc, evchunk[(size_t)4 * c + 2], evchunk[(size_t)4 * c + 3]));
      km += kr;
      kg += kc;
    }
  } else {
    HIPCHK(hipEventElapsedTime(&km, ev0, evm));
    kg = k1 - km;
  }
  row_ms += km;
  gram_ms += kg;
  return SGLM_OK;
}

int sglm_engine::blas_handle() {
  if (!blas) {
    if (rocblas_create_handle(&blas) != rocblas_status_success) {
      blas = nullptr;
      set_error("rocblas_create_handle failed");
      return SGLM_EHIP;
    }
  }
  if (rocblas_set_stream(blas, st) != rocblas_status_success) {
    set_error("rocblas_set_stream failed");
    return SGLM_EHIP;
  }
  return SGLM_OK;
}

// =====================================================================================
// Device solver for wide p, from the reduced buffer on the GPU.
// Default: Cholesky (rocSOLVER potrf / potrs, potri for the standard errors).  A matrix potrf
// rejects or whose pivots flag it ill-conditioned (solve.hpp LU_SWITCH_RATIO) takes the
// reference's own algorithm, LU with partial pivoting and the explicit inverse (Breeze inv =
// LAPACK dgetrf + dgetri, utils.scala:103-105, 134-136): on the host -- the oracle's unblocked
// order, as the narrow path -- up to p = HOST_LU_MAX_P, by rocSOLVER getrf / getri above it (a
// host LU at p = 2048 is ~10 s).  SGLM_WIDE_SOLVE=lu runs the rocSOLVER LU route always, coefs =
// inv * X'Wz summed in the reference's order (inv_gemv_kernel), stdErr from diag(inv).
// Measured against the oracle's unblocked LU (tests/test_gpu_wide.py, oracle/lu_floor.py):
// Cholesky lands closer than rocSOLVER's blocked getrf + getri on ill-conditioned gamma designs
// (p = 520, cond ~1e7: 1e-9 against 1e-7 elementwise on the smallest coefficient), which is why
// it stays the default; norm-wise both agree to ~1e-12.  Exact singularity (a zero pivot of
// dgetrf) -> MatrixSingularException, as Breeze's inv.
// =====================================================================================
namespace {

constexpr int64_t HOST_LU_MAX_P = 1024;

struct DeviceSolver : public SolverIface {
  sglm_engine* e;
  int64_t p;
  double *dA = nullptr, *dB = nullptr, *dAi = nullptr, *dpk = nullptr, *dx = nullptr;
  rocblas_int *dinfo = nullptr, *dipiv = nullptr;
  std::vector<double> ldiag;
  std::unique_ptr<HostSolver> host;
  int kind = 0;  // 0 none, 1 Cholesky factor in dA, 2 explicit inverse in dA (LU route), 3 host solver
  DeviceSolver(sglm_engine* eng, int64_t pp) : e(eng), p(pp) {}
  int path() const override {
    return kind == 1 ? SGLM_SOLVE_DEVICE_CHOL : kind == 2 ? SGLM_SOLVE_DEVICE_LU : kind == 3 ? host->path() : -1;
  }
  ~DeviceSolver() override {
    (void)hipSetDevice(e->device);
    sglm_engine::dev_free({&dA, &dB, &dAi, &dpk, &dx});
    if (dinfo) (void)hipFree(dinfo);
    if (dipiv) (void)hipFree(dipiv);
  }
  int alloc() {
    if (dA) return SGLM_OK;
    HIPCHK(hipMalloc(&dA, sizeof(double) * (size_t)(p * p)));
    HIPCHK(hipMalloc(&dAi, sizeof(double) * (size_t)(p * p)));
    HIPCHK(hipMalloc(&dB, sizeof(double) * (size_t)p));
    HIPCHK(hipMalloc(&dx, sizeof(double) * (size_t)p));
    HIPCHK(hipMalloc(&dinfo, sizeof(rocblas_int)));
    HIPCHK(hipMalloc(&dipiv, sizeof(rocblas_int) * (size_t)p));
    return SGLM_OK;
  }
  int read_info(rocblas_int* info) {
    HIPCHK(hipMemcpyAsync(info, dinfo, sizeof *info, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    return SGLM_OK;
  }
  int solve(const double* packed, double* x) override {
    HIPCHK(hipSetDevice(e->device));
    int rc = alloc();
    if (!rc) rc = e->blas_handle();
    if (rc) return rc;
    const double* src = e->dred;
    if (!e->red_on_device) {  // the reduction ended on the host: upload it
      if (!dpk) HIPCHK(hipMalloc(&dpk, sizeof(double) * (size_t)packed_len(p)));
      HIPCHK(hipMemcpyAsync(dpk, packed, sizeof(double) * (size_t)packed_len(p), hipMemcpyHostToDevice, e->st));
      src = dpk;
    }
    kind = 0;
    if (e->wide_lu) return solve_lu(src, x);
    HIPCHK(launch_unpack_lower(src, (int)p, dA, dB, e->st));
    if (rocsolver_dpotrf(e->blas, rocblas_fill_lower, (rocblas_int)p, dA, (rocblas_int)p, dinfo) !=
        rocblas_status_success) {
      set_error("rocsolver_dpotrf failed");
      return SGLM_EHIP;
    }
    rocblas_int info = 0;
    HIPCHK(hipMemcpyAsync(&info, dinfo, sizeof info, hipMemcpyDeviceToHost, e->st));
    if (info == 0) {  // diag(L) for the collinearity check (solve.hpp chol_pivot_ratio)
      ldiag.resize((size_t)p);
      HIPCHK(hipMemcpy2DAsync(ldiag.data(), sizeof(double), dA, sizeof(double) * (size_t)(p + 1), sizeof(double),
                              (size_t)p, hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(hipStreamSynchronize(e->st));
    if (info == 0) {
      double r = 1.0;
      for (int64_t j = 0; j < p; ++j) {
        const double a = packed[j * (j + 1) / 2 + j];
        if (a > 0.0) r = std::fmin(r, ldiag[(size_t)j] * ldiag[(size_t)j] / a);
      }
      if (r < LU_SWITCH_RATIO) info = -1;  // ill-conditioned: the reference's LU inverse
    }
    if (info != 0) {  // not positive definite / ill-conditioned: the reference's LU inverse
      if (p > HOST_LU_MAX_P) return solve_lu(src, x);
      if (!host) host = std::make_unique<HostSolver>(p);
      kind = 3;
      return host->solve(packed, x);
    }
    if (rocsolver_dpotrs(e->blas, rocblas_fill_lower, (rocblas_int)p, 1, dA, (rocblas_int)p, dB, (rocblas_int)p) !=
        rocblas_status_success) {
      set_error("rocsolver_dpotrs failed");
      return SGLM_EHIP;
    }
    HIPCHK(hipMemcpyAsync(x, dB, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    kind = 1;
    return SGLM_OK;
  }
  // inv(A) by dgetrf + dgetri in dA, x = inv(A) b (utils.scala:103-104)
  int solve_lu(const double* src, double* x) {
    HIPCHK(launch_unpack_lower(src, (int)p, dA, dB, e->st, true));
    if (rocsolver_dgetrf(e->blas, (rocblas_int)p, (rocblas_int)p, dA, (rocblas_int)p, dipiv, dinfo) !=
        rocblas_status_success) {
      set_error("rocsolver_dgetrf failed");
      return SGLM_EHIP;
    }
    rocblas_int info = 0;
    if (int rc = read_info(&info)) return rc;
    if (info != 0) {
      set_error("breeze.linalg.MatrixSingularException: X'WX is singular");
      return SGLM_ESINGULAR;
    }
    if (rocsolver_dgetri(e->blas, (rocblas_int)p, dA, (rocblas_int)p, dipiv, dinfo) != rocblas_status_success) {
      set_error("rocsolver_dgetri failed");
      return SGLM_EHIP;
    }
    HIPCHK(launch_inv_gemv(dA, (int)p, dB, dx, e->st));
    HIPCHK(hipMemcpyAsync(x, dx, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, e->st));
    if (int rc = read_info(&info)) return rc;
    if (info != 0) {
      set_error("breeze.linalg.MatrixSingularException: X'WX is singular");
      return SGLM_ESINGULAR;
    }
    kind = 2;
    return SGLM_OK;
  }
  // inv(A) (lower triangle) into dAi from the kept Cholesky factor
  int device_inverse() {
    HIPCHK(hipMemcpyAsync(dAi, dA, sizeof(double) * (size_t)(p * p), hipMemcpyDeviceToDevice, e->st));
    if (rocsolver_dpotri(e->blas, rocblas_fill_lower, (rocblas_int)p, dAi, (rocblas_int)p, dinfo) !=
        rocblas_status_success) {
      set_error("rocsolver_dpotri failed");
      return SGLM_EHIP;
    }
    return SGLM_OK;
  }
  int inv_diag(double* d) override {
    if (kind == 3) return host->inv_diag(d);
    if (kind == 0) {
      for (int64_t i = 0; i < p; ++i) d[i] = 0.0;
      return SGLM_OK;
    }
    HIPCHK(hipSetDevice(e->device));
    if (kind == 1)
      if (int rc = device_inverse()) return rc;
    HIPCHK(hipMemcpy2DAsync(d, sizeof(double), kind == 1 ? dAi : dA, sizeof(double) * (size_t)(p + 1), sizeof(double),
                            (size_t)p, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    return SGLM_OK;
  }
  int inverse(double* Ainv) override {
    if (kind == 3) return host->inverse(Ainv);
    if (kind == 0) return SGLM_OK;
    HIPCHK(hipSetDevice(e->device));
    if (kind == 1)
      if (int rc = device_inverse()) return rc;
    HIPCHK(hipMemcpyAsync(Ainv, kind == 1 ? dAi : dA, sizeof(double) * (size_t)(p * p), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    if (kind == 1)
      for (int64_t j = 0; j < p; ++j)
        for (int64_t i = 0; i < j; ++i) Ainv[i + j * p] = Ainv[j + i * p];
    return SGLM_OK;
  }
};

}  // namespace

std::unique_ptr<SolverIface> sglm_engine::make_solver(int64_t pp) {
  if (group()) return subs[0]->make_solver(pp);
  if (wide) return std::make_unique<DeviceSolver>(this, pp);
  return std::make_unique<HostSolver>(pp);
}
