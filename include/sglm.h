/*
 * sglm.h -- C ABI of the MI355X fitting engine for sparkGLM's lm()/glm() hot path.
 *
 * This is the drop-in boundary.  The reference (cafreeman/sparkGLM, Scala/Spark) has no
 * FFI of its own; the seam is internal: the fit drivers return PreGLM / PreLM and the
 * unchanged model code (GLM.createObj, new LM) builds the user-visible objects.  Each
 * entry point below replaces one reference function body, reached from Scala over JNI
 * (binding stubs in INTEGRATION.md):
 *
 *   sglm_set_data        replaces utils.dataFrameToMatrix / dfToDenseMatrix
 *                        (utils.scala:36-49) + the per-action re-conversion: one upload,
 *                        X stays resident in HBM across iterations and fits.
 *   sglm_reserve +       the same, partition by partition (dataFrameToMatrix builds one
 *   sglm_set_rows        DenseMatrix per partition, utils.scala:36-39; GLM.scala:576-578):
 *                        blocks of rows -- each within a JVM array's 2^31 elements -- staged
 *                        through pinned buffers into the reserved shard.
 *   sglm_fit_glm         replaces GLM.fitSingleBinomial (GLM.scala:254-315) and
 *                        GLM.fitMultipleBinomial (GLM.scala:410-468); output = PreGLM
 *                        (GLM.scala:25-33).
 *   sglm_fit_lm          replaces LM.fitSingle / LM.fitMultiple (LM.scala:191-237) and
 *                        the stderr tail of LM.fit (LM.scala:260-263); output = PreLM
 *                        (LM.scala:10-14) + stdErr/sigma.
 *   sglm_irls_pass       one IRLS pass (zwCreateBinomial + wlsComponents, GLM.scala:
 *                        359-395, utils.scala:110-126) for tests and benchmarks.
 *   sglm_predict_new     replaces LM.predictSingle/predictMultiple's newX * coefs
 *                        (LM.scala:39-61) on new rows, without evicting the resident shard;
 *                        response scale (mu = unlink(eta)) for GLMs.
 *   sglm_create          SURVEY 8(b)'s constructor over devs[0..ndev): one device, or one
 *                        process owning several GPUs (the single Spark driver that calls
 *                        GLM.fit / LM.fit, GLM.scala:587, LM.scala:254): row shards per device,
 *                        one RCCL group all-reduce (ncclCommInitAll) per iteration.
 *   sglm_glm_summary / sglm_lm_summary
 *                        the printed summaries of GLM.summary (GLM.scala:998-1025) and
 *                        SummaryLM (LM.scala:66-137), produced host-side in C++.
 *
 * Conventions
 *   - Status codes: 0 ok; SGLM_EINVAL maps to IllegalArgumentException (the reference's
 *     require(...)); SGLM_ESINGULAR to breeze MatrixSingularException; SGLM_EHIP /
 *     SGLM_ECOMM to RuntimeException.  sglm_last_error() returns a thread-local message.
 *   - Matrices are column-major fp64 (Breeze DenseMatrix layout): element (i,j) at
 *     X[i + j*ldx].  The caller keeps ownership of every pointer it passes; the engine
 *     copies into device memory it owns until sglm_destroy.
 *   - A handle from sglm_create with ndev = 1 (or sglm_create_device) drives one HIP device;
 *     with ndev > 1 it drives several (row shards, Spark's slicing [d n/D, (d+1) n/D)).  Across processes (or host
 *     threads, one handle each) shards join a communicator: RCCL over xGMI, a caller-supplied
 *     all-reduce, or the in-process sglm_local_allreduce.  Every rank receives identical results.
 *   - Handles are not thread-safe; distinct handles may be used concurrently.
 */
#ifndef SGLM_H
#define SGLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGLM_ABI_VERSION 8  /* 3: sglm_stats.dev_passes; 4: sglm_stats.overlap_chunks; 5: sglm_set_comm_rank,
                              sglm_stats.comm_path / rank_blocks / pass_kernel_ms_min / proc_chunks /
                              proc_chunk_rows / solve_path; 6: sglm_stats.pass_kernel / pass_kernel_name,
                              sglm_set_comm_rank collective; 7: sglm_stats.lm_device_fits /
                              lm_device_reruns; 8: sglm_create(devs, ndev) as SURVEY 8(b) names it,
                              the one-device form renamed sglm_create_device (sglm_create_multi stays:
                              the group handle at any ndev), SGLM_KERNEL_NARROW_SPLIT retired,
                              sglm_stats.lm_onepass_fits.  Added since, without a version change (new
                              symbols only): sglm_vcov, sglm_influence, sglm_predict_new_se,
                              sglm_get_influence_ms, enum sglm_resid_type, sglm_vcov_robust,
                              sglm_get_sandwich_ms, enum sglm_hc_type, sglm_set_clusters, sglm_vcov_cluster,
                              sglm_get_cluster_ms, sglm_cluster_plan, sglm_set_theta, sglm_get_theta,
                              sglm_get_theta_ms, sglm_nb_theta_terms, sglm_theta_ml, sglm_fit_glm_start, sglm_fit_glm_nb
                              (with sglm_nb_opts / sglm_nb_result), sglm_fit_glm_fe (with sglm_fe_info),
                              sglm_fe_pass, sglm_vcov_fe, sglm_get_fe_ms, sglm_set_fe2, sglm_fe2_plan,
                              sglm_fit_glm_fe2 (with sglm_fe2_opts / sglm_fe2_info), sglm_fe2_pass,
                              sglm_vcov_fe2, sglm_get_fe2_ms, sglm_fit_glm_gee (with sglm_gee_opts /
                              sglm_gee_info, enum sglm_corstr), sglm_gee_pass, sglm_vcov_gee,
                              sglm_get_gee_ms, sglm_fit_glm_firth (with sglm_firth_opts / sglm_firth_info),
                              sglm_firth_pass, sglm_get_firth_ms, sglm_fit_multinom (with sglm_multinom_opts /
                              sglm_multinom_info), sglm_multinom_pass, sglm_get_multinom_ms;
                              (new values only:) SGLM_SQRT and
                              the non-canonical (family, link) pairs of enum sglm_link's table,
                              SGLM_NEGBIN and its three pairs */

enum sglm_status {
  SGLM_OK = 0,
  SGLM_EINVAL = 1,    /* require(...) failed -> IllegalArgumentException */
  SGLM_ESINGULAR = 2, /* inv() of a singular matrix -> MatrixSingularException */
  SGLM_EHIP = 3,      /* HIP runtime / device error */
  SGLM_ECOMM = 4,     /* RCCL or caller all-reduce failure */
  SGLM_ENOMEM = 5     /* device or host allocation failed */
};

/* Families: the reference fits only binomial (GLM.scala:486-590); the rest follow R's
 * family objects on the reference's IRLS skeleton. */
enum sglm_family { SGLM_BINOMIAL = 0, SGLM_GAUSSIAN = 1, SGLM_POISSON = 2, SGLM_GAMMA = 3, SGLM_NEGBIN = 4 };
/* The (family, link) pairs, R's three links per family; any other pair is SGLM_EINVAL:
 *   binomial  logit, probit, cloglog
 *   gaussian  identity, log, inverse
 *   poisson   log, identity, sqrt
 *   gamma     inverse, identity, log
 *   negbin    log, sqrt, identity      (MASS::negative.binomial(theta): V = mu + mu^2 / theta)
 * The negative binomial's theta is not in sglm_glm_opts: it lives on the handle (sglm_set_theta, or estimated
 * by sglm_fit_glm_nb).  Every call that takes SGLM_NEGBIN on a handle whose theta was never set is
 * SGLM_EINVAL.  None of its links is canonical: its rows follow the poisson rows' validity rule below.
 * With a non-canonical link of gaussian / poisson / gamma the mean can leave the family's range during
 * the iterations (R's validmu / valideta: poisson and gamma need mu finite and > 0, sqrt eta > 0; gaussian
 * eta finite, inverse eta != 0).  There is no step-halving: such a fit returns SGLM_EINVAL ("no valid set
 * of coefficients: mu left the poisson range at iteration k"), and sglm_irls_pass returns a non-finite
 * scalars[0]. */
enum sglm_link {
  SGLM_LOGIT = 0, SGLM_PROBIT = 1, SGLM_CLOGLOG = 2, /* binomial (GLM.scala:190-251) */
  SGLM_IDENTITY = 3, SGLM_LOG = 4, SGLM_INVERSE = 5,  /* gaussian / poisson / gamma */
  SGLM_SQRT = 6                                       /* poisson, negbin */
};

/* How mu is formed on the first iteration. */
enum sglm_init {
  SGLM_INIT_SINGLE = 0,  /* fitSingleBinomial: mu = mean(y) directly (GLM.scala:263, 282-290) */
  SGLM_INIT_MULTIPLE = 1 /* fitMultipleBinomial: mu = unlink(link(mean(y))) (GLM.scala:370-371) */
};

/* How the last p x p solve ran (sglm_stats.solve_path). */
enum sglm_solve_path {
  SGLM_SOLVE_HOST_CHOL = 0,   /* host Cholesky (p <= 256, well conditioned) */
  SGLM_SOLVE_HOST_LU = 1,     /* host LU + explicit inverse: Breeze inv (utils.scala:103-105) */
  SGLM_SOLVE_DEVICE_CHOL = 2, /* wide p (default): rocSOLVER potrf / potrs / potri */
  SGLM_SOLVE_DEVICE_LU = 3    /* wide p, SGLM_WIDE_SOLVE=lu (or ill-conditioned above p = 1024):
                                 rocSOLVER getrf + getri, coefs = inv * X'Wz */
};

/* Where a pass's all-reduce ran (sglm_stats.comm_path). */
enum sglm_comm_path {
  SGLM_COMM_NONE = 0,         /* one shard, no communicator */
  SGLM_COMM_CALLER_HOST = 1,  /* sglm_set_comm, host buffers (gloo, sglm_local_allreduce, ...) */
  SGLM_COMM_CALLER_DEVICE = 2,/* sglm_set_comm, device buffers (e.g. a torch RCCL group) */
  SGLM_COMM_RCCL = 3,         /* sglm_set_comm_rccl: the engine's own RCCL communicator (xGMI) */
  SGLM_COMM_GROUP_RCCL = 4,   /* multi-device handle: one RCCL group call over ncclCommInitAll */
  SGLM_COMM_GROUP_HOST = 5    /* multi-device handle with a repeated device: host sums in shard order */
};

/* The kernel that ran the last pass (sglm_stats.pass_kernel; the roofline line's `kernel`). */
enum sglm_pass_kernel {
  SGLM_KERNEL_NONE = 0,
  SGLM_KERNEL_FUSED = 1,       /* irls_pass_kernel<P16, fam, link>: 65 <= p <= 256 below the K1r threshold */
  SGLM_KERNEL_FUSED_SPLIT = 2, /* irls_pass_r_kernel<P16, fam, link> (K1r, split roles) */
  SGLM_KERNEL_NARROW = 3,      /* irls_narrow_kernel<P16, fam, link, irls, stats>: p <= 64 */
  SGLM_KERNEL_WIDE = 4,        /* wide_rows_kernel + wide_gram_kernel: p > 256 (resident X) */
  SGLM_KERNEL_WIDE_PROC = 5    /* the same over procedural X (generated chunks or in-kernel) */
  /* 6 (SGLM_KERNEL_NARROW_SPLIT, ABI <= 7): retired with its kernel, never returned */
};

/* Prediction scale (R's predict(type = "link" | "response")). */
enum sglm_predict_type { SGLM_PREDICT_LINK = 0, SGLM_PREDICT_RESPONSE = 1 };

typedef struct sglm_engine sglm_engine;

typedef struct {
  int family;      /* enum sglm_family */
  int link;        /* enum sglm_link */
  double tol;      /* absolute |delta deviance| stopping tolerance; reference default 1e-6 */
  int verbose;     /* print "iter\tdeltad" per iteration (GLM.scala:304, 461) */
  int max_iter;    /* 0 = unbounded, as in the reference (extension guard otherwise) */
  int init_mode;   /* enum sglm_init */
  int npart;       /* value reported in PreGLM.npart (reference: Spark partition count); 0 = #ranks */
} sglm_glm_opts;

typedef struct { /* PreGLM (GLM.scala:25-33) */
  double *coefs;        /* [p] caller-allocated */
  double *std_err;      /* [p] caller-allocated: sqrt(diag(inv(X'WX))) of the last solve */
  double deviance;
  double null_deviance;
  double pearson;
  double loglik;
  int iter;
  double nrow;
  int npart;
  double *dev_trace;    /* optional [max_trace]: deviance after each iteration, [0] = null */
  int max_trace;
} sglm_preglm;

typedef struct { /* PreLM (LM.scala:10-14) + LM.fit's derived stdErr / sigma */
  double *coefs;        /* [p] */
  double *xtxi;         /* [p*p] col-major inv(X'X), may be NULL */
  double *std_err;      /* [p] sqrt(sse/(n-p) * diag(xtxi)) (LM.scala:260-263) */
  double sse;
  double r2;            /* SSR/SST, as the reference (LM.scala:185) */
  double fstat;
  double sigma;
  double nrow;
  int npart;
} sglm_prelm;

/* Per-handle timing counters (HIP events on the engine stream). */
typedef struct {
  int64_t passes;           /* fused IRLS / LM passes launched */
  double pass_kernel_ms;    /* total time of the fused pass kernel (sum over passes) */
  double reduce_kernel_ms;  /* total time of the partial-reduction kernel */
  double last_pass_ms;      /* fused kernel time of the last pass */
  double comm_ms;           /* host wall time in the all-reduce */
  double solve_ms;          /* host wall time in the p x p solves */
  int64_t n_local;          /* rows resident on this device */
  int64_t p;
  int workgroups;           /* fused-kernel grid size (wide path: Gram work items) */
  int kernel_variant;       /* fused path: column-block count P16; wide path: 0 */
  int path;                 /* 0 fused single-panel pass (p <= 256), 1 wide panel-pair pass */
  int wide_panels;          /* wide path: 128-column panels */
  double row_kernel_ms;     /* wide path: total time of the row kernel (eta, w, w*z) */
  double gram_kernel_ms;    /* wide path: total time of the panel-pair Gram kernel */
  double load_ms;           /* host wall time of set_data / set_rows (pinned staging + H2D) */
  int64_t load_bytes;       /* bytes those calls moved to the device */
  int ndev;                 /* devices driven by this handle */
  int rccl_group;           /* multi-device handle reducing over RCCL (1) or on the host (0) */
  int64_t dev_passes;       /* deviance-only passes: iterations the fit predicted to be its last
                               (quadratic convergence) ran without the unused Gram; bitwise the
                               scalars of the full pass (SGLM_SPECULATE=0 disables) */
  int overlap_chunks;       /* wide path, resident X: chunks per pass whose row kernel runs on a
                               second stream beside the previous chunk's Gram (0: not overlapped;
                               SGLM_WIDE_OVERLAP sets the count, SGLM_WIDE_OV_MIN the fewest rows) */
  int comm_path;            /* enum sglm_comm_path */
  int rank_blocks;          /* 1: the scalars (deviance, ...) are summed across ranks / shards in rank
                               order with compensation from per-rank blocks (needs the own rank: RCCL,
                               the in-process communicator, or sglm_set_comm_rank); 0: plain sum */
  double pass_kernel_ms_min;/* multi-device handle: pass_kernel_ms of the fastest shard (the max is
                               pass_kernel_ms); one device: = pass_kernel_ms.  comm_ms there is
                               the collective after the last shard arrived (RCCL: device events) */
  int proc_chunks;          /* procedural shard: chunks of X generated per pass (0: in-kernel) */
  int64_t proc_chunk_rows;  /* rows per chunk (SGLM_PROC_SCRATCH_MAX caps the scratch, GiB) */
  int solve_path;           /* enum sglm_solve_path of the last solve, -1 before any */
  int pass_kernel;          /* enum sglm_pass_kernel of the last pass (the engine's own choice: the K1 / K1r
                               threshold, its row limit, the narrow / wide paths) */
  char pass_kernel_name[64];/* that kernel's name as rocprofv3 lists it, e.g. "irls_pass_r_kernel<16,binomial,logit>";
                             the link slot reads "runtime" for the pairs that run their family's run-time-link
                             instantiation (every non-canonical pair but gamma / log) */
  int64_t lm_device_fits;   /* LM fits done in one device round trip (Gram pass, device Cholesky, residual pass;
                               resident p <= 64 shards without a communicator; SGLM_LM_DEVICE=0 disables) */
  int64_t lm_device_reruns; /* of those, fits whose device coefficients were not the host solve's bit for bit (the
                               host left Cholesky for LU) or whose one-pass statistics were flagged: the residual
                               pass reran at the host's coefficients */
  int64_t lm_onepass_fits;  /* of the device fits, those whose SSE / R^2 / F came from the Gram pass's sums (X'X,
                               X'y, X'1, y'y, sum y) -- one pass over X -- instead of a residual pass */
} sglm_stats;

/* Caller-supplied all-reduce (sum, fp64, in place).  on_device != 0: buf is a device
 * pointer and stream the engine's hipStream_t; otherwise buf is host memory.
 * THREAD: with a deadline (SGLM_COMM_TIMEOUT_S > 0, the default 300 s, read when the communicator
 * is set) the callback runs on a communicator thread the handle owns (its device current), not on
 * the thread that called sglm_fit_* / sglm_irls_*, which waits with the deadline; a callback still
 * running at the deadline is abandoned on that thread.  Callbacks bound to the calling thread
 * (MPI_THREAD_SINGLE / FUNNELED, thread-local JNI or torch state) need SGLM_COMM_TIMEOUT_S=0: the
 * callback then runs inline on the caller's thread, without a deadline.  sglm_local_allreduce
 * always runs inline (it bounds its own wait). */
typedef int (*sglm_allreduce_fn)(void *ctx, double *buf, int64_t count, void *stream, int on_device);

/* ---- lifecycle ---------------------------------------------------------------- */
int sglm_abi_version(void);
const char *sglm_last_error(void);
int sglm_device_count(int *count);
/* One handle over devs[0..ndev).  ndev = 1: a single-device handle, exactly
 * sglm_create_device(devs[0]).  ndev > 1: rows are sharded contiguously across the devices; each
 * iteration's packed partials are all-reduced by one RCCL group call over communicators from
 * ncclCommInitAll (distinct devices) or summed on the host in device order (a device listed
 * twice: rehearsal on fewer GPUs).  Every call below accepts a multi-device handle, except
 * sglm_set_data_device, sglm_set_comm and sglm_set_comm_rccl. */
int sglm_create(const int *devs, int ndev, sglm_engine **out);
/* One device by ordinal (the ABI <= 7 sglm_create(int, ...)). */
int sglm_create_device(int device, sglm_engine **out);
/* Always the multi-device (group) handle, for ndev = 1 too: a one-device group runs the RCCL
 * group all-reduce path (ncclCommInitAll over one device) -- how tests execute it on one GPU. */
int sglm_create_multi(const int *devs, int ndev, sglm_engine **out);
int sglm_handle_devices(sglm_engine *h, int *ndev);
void sglm_destroy(sglm_engine *h);

/* ---- data (utils.dataFrameToMatrix replacement) ------------------------------ */
/* Host arrays.  m (binomial trials), offset and prior (weights) may be NULL. */
int sglm_set_data(sglm_engine *h, const double *X, int64_t n, int64_t p, int64_t ldx,
                  const double *y, const double *m, const double *offset, const double *prior);
/* Same, from device memory already on this engine's device. */
int sglm_set_data_device(sglm_engine *h, const double *dX, int64_t n, int64_t p, int64_t ldx,
                         const double *dy, const double *dm, const double *doffset,
                         const double *dprior);
/* Partition-wise ingest.  sglm_reserve allocates the shard (n rows x p columns, plus the
 * optional vectors) without filling it; sglm_set_rows then copies rows [row0, row0+nrows)
 * from a host column-major block (leading dimension ldx >= nrows; vectors of nrows) through
 * two pinned staging buffers (pageable memory never reaches the DMA engine).  Blocks may
 * arrive in any order and must not overlap; a fit requires every reserved row written.
 * m / offset / prior must be passed exactly when reserved. */
int sglm_reserve(sglm_engine *h, int64_t n, int64_t p, int has_m, int has_offset, int has_prior);
int sglm_set_rows(sglm_engine *h, int64_t row0, int64_t nrows, const double *X, int64_t ldx,
                  const double *y, const double *m, const double *offset, const double *prior);
/* Generate this rank's row shard [row0, row0+n) of the seeded synthetic design directly
 * in HBM (bench / scale tests).  kind: 0 = logit design (y in {0,1}), 1 = gaussian (LM),
 * 2 = poisson counts + offset + prior, 3 = gamma design (positive X, y > 0).  Column 0
 * is the intercept.  Bit-identical to sparkglm_amd.synth on the host. */
int sglm_synth(sglm_engine *h, int kind, int64_t row0, int64_t n, int64_t p, uint64_t seed);
/* Procedural shard of the same synthetic design: y (+ offset / prior for kind 2) are
 * generated and stored, X is NOT -- the (wide-path) pass kernels regenerate every X[i, j]
 * from the counter-based generator where they would have read it, bit-identical to the
 * resident image of sglm_synth.  For designs larger than HBM (BASELINE configs[4]:
 * 2B x 512 = 8.19 TB).  Fits, LM, predict and stats work as on a resident shard;
 * sglm_get_data cannot return X. */
int sglm_synth_procedural(sglm_engine *h, int kind, int64_t row0, int64_t n, int64_t p, uint64_t seed);
/* Copy back the resident design (tests; X col-major with ldx = n). */
int sglm_get_data(sglm_engine *h, double *X, double *y, double *m, double *offset, double *prior);

/* ---- communicators (Spark treeReduce replacement) ----------------------------- */
/* fn runs on the handle's communicator thread unless SGLM_COMM_TIMEOUT_S=0 (see sglm_allreduce_fn).
 * RCCL (sglm_set_comm_rccl) and group handles: the deadline of an all-reduce starts when the work
 * this rank queued before it (its pass kernels) has finished, so it bounds the wait for the peers only. */
int sglm_set_comm(sglm_engine *h, sglm_allreduce_fn fn, void *ctx, int on_device);
/* This handle's rank in the communicator just set by sglm_set_comm (0 <= rank < its rank count;
 * known without this call for RCCL and sglm_local_allreduce).  With it the per-iteration scalars
 * (deviance, Pearson, loglik) are summed across ranks in rank order with compensation, so the
 * convergence test does not depend on the rank count beyond ~1 ulp.  COLLECTIVE: every rank of the
 * communicator calls it (it changes the length of every later all-reduce); one all-reduce checks
 * that all ranks joined with distinct ranks, else SGLM_EINVAL on every rank. */
int sglm_set_comm_rank(sglm_engine *h, int rank);
/* Native RCCL communicator over xGMI.  unique_id: 128 bytes from
 * sglm_rccl_unique_id() on rank 0, broadcast by the caller. */
int sglm_rccl_unique_id(void *out128);
int sglm_set_comm_rccl(sglm_engine *h, int nranks, int rank, const void *unique_id128);

/* ---- fits ---------------------------------------------------------------------- */
int sglm_fit_glm(sglm_engine *h, const sglm_glm_opts *opts, sglm_preglm *out);
int sglm_fit_lm(sglm_engine *h, sglm_prelm *out);
/* sglm_fit_glm warm-started (R's start=): the initial constant-mu pass is replaced by a pass at beta_start
 * [p].  dev_trace[0] is the deviance at beta_start; the loop and its stop rule |delta deviance| <= tol are
 * sglm_fit_glm's; iter counts solves; null_deviance comes from one initial-mode pass at mean(y).  Every
 * family. */
int sglm_fit_glm_start(sglm_engine *h, const sglm_glm_opts *opts, const double *beta_start, sglm_preglm *out);

/* ---- negative binomial --------------------------------------------------------- */
/* theta of SGLM_NEGBIN on this handle (a group handle: on all its shards).  theta <= 0 or non-finite is
 * SGLM_EINVAL.  sglm_get_theta returns 0 while none was set.  Ranks of a communicator each set their own
 * handle (sglm_fit_glm_nb leaves the identical value on every rank). */
int sglm_set_theta(sglm_engine *h, double theta);
int sglm_get_theta(sglm_engine *h, double *theta);
/* theta_terms_kernel launches on this handle since it was created and their summed kernel time (HIP events; a
 * multi-device handle: its slowest shard). */
int sglm_get_theta_ms(sglm_engine *h, int64_t *launches, double *kernel_ms);
/* The theta score, information and log-likelihood at beta [p] and theta, with mu = unlink(X beta + offset), w
 * the prior weight: out[5] = {
 *   sum w [psi(theta+y) - psi(theta) + log theta + 1 - log(theta+mu) - (y+theta)/(mu+theta)],
 *   sum w [-psi'(theta+y) + psi'(theta) - 1/theta + 2/(mu+theta) - (y+theta)/(mu+theta)^2],
 *   sum w dnbinom(y, theta, mu, log), sum w (y/mu - 1)^2, sum w }.
 * opts: the link (family ignored).  It first forms eta at beta with one deviance-only pass (no Gram), then
 * runs one streaming kernel over y, eta and the prior weights.  COLLECTIVE over a communicator; every rank
 * gets bitwise the same sums (rank blocks, compensated, as the pass scalars). */
int sglm_nb_theta_terms(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, double theta, double *out5);
/* MASS::theta.ml at beta: t0 = sum w / sum w (y/mu - 1)^2; it = 0; del = 1;
 *   while (++it < limit && |del| > eps) { t0 = |t0|; del = score(t0) / info(t0); t0 += del; }
 * *theta = t0 (0 where t0 < 0), *se = sqrt(1 / info) of the last step, *iters = it, *warn: bit 0 "iteration
 * limit reached" (it == limit), bit 1 "estimate truncated at zero".  limit <= 0: 25; eps <= 0: 2^-13
 * (.Machine$double.eps^0.25).  Each Newton step is one kernel launch and one all-reduce of five scalars.
 * The handle's theta is not changed.  COLLECTIVE. */
int sglm_theta_ml(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, int limit, double eps,
                  double *theta, double *se, int *iters, int *warn);
typedef struct {
  int maxit;         /* outer alternations; 0: 25 */
  double epsilon;    /* outer stop |Lm0 - Lm| / d1 + |del| <= epsilon; 0: 1e-8 */
  int theta_limit;   /* sglm_theta_ml's limit; 0: 25 */
  double theta_eps;  /* sglm_theta_ml's eps; 0: 2^-13 */
} sglm_nb_opts;
typedef struct {
  double theta, se_theta, twologlik;
  int outer_iter;    /* inner negative binomial fits run */
  int theta_warn;    /* the last sglm_theta_ml's warn bits */
  int converged;     /* 0: maxit ended the alternation */
} sglm_nb_result;
/* MASS::glm.nb: a Poisson fit (opts->link, opts->init_mode, opts->tol), theta by sglm_theta_ml, then
 * alternately a negative binomial fit at theta warm-started from the last coefficients (sglm_fit_glm_start)
 * and theta by sglm_theta_ml at its coefficients, until |Lm0 - Lm| / d1 + |theta_old - theta| <= epsilon
 * (Lm = twice the log-likelihood, d1 = sqrt(2 max(1, n - p))).  opts->family is ignored.  `out` is the last
 * inner fit; its null_deviance is recomputed at the final theta and its loglik is twologlik / 2.  The final
 * theta stays set on the handle, so sglm_vcov*, sglm_influence and sglm_predict_* with SGLM_NEGBIN follow
 * without another call.  A failure of an inner fit is returned as that fit's status.  nb_opts may be NULL
 * (all defaults).  COLLECTIVE. */
int sglm_fit_glm_nb(sglm_engine *h, const sglm_glm_opts *opts, const sglm_nb_opts *nb_opts, sglm_preglm *out,
                    sglm_nb_result *nb);

/* One IRLS pass at beta (beta == NULL: the initial constant-eta pass at mu0),
 * all-reduced over the communicator.  Outputs (any may be NULL): gram [p*p] col-major
 * full symmetric X'WX, xtwz [p], scalars [8] = {deviance-sum, pearson, loglik-part, bad,
 * aux0, aux1, aux2, sum prior}. */
int sglm_irls_pass(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, double mu0,
                   double *gram, double *xtwz, double *scalars);

/* The test-level step of SURVEY.md 8(b): the pass at beta (beta != NULL) with the deviance at
 * beta (family factor applied, as GLM.scala:397 createBinomialDeviance sums it).  Outputs may be
 * NULL: xtwx [p*p] col-major full symmetric X'WX, xtwz [p], dev. */
int sglm_irls_step(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, double *xtwx, double *xtwz,
                   double *dev);

/* `iters` IRLS iterations from beta (in/out): each is one fused pass at beta followed by
 * the p x p solve -- the unit the benchmark times.  last_dev (may be NULL) receives the
 * deviance at the last input beta. */
int sglm_irls_iterations(sglm_engine *h, const sglm_glm_opts *opts, double *beta, int iters,
                         double *last_dev);

/* eta = X * beta (+ offset if add_offset) for the resident rows, written to out [n_local]. */
int sglm_predict(sglm_engine *h, const double *beta, int add_offset, double *out);
/* The same on the link (eta) or response (mu = unlink(eta, m), m = the resident trials or 1)
 * scale of family/link: fitted values of the resident rows. */
int sglm_predict_glm(sglm_engine *h, const double *beta, int family, int link, int type, int add_offset,
                     double *out);
/* Score NEW rows (LM.predict, LM.scala:29-61; GLM response-scale prediction): X column-major
 * n x p (ldx >= n), optional offset / m (NULL: 0 / 1).  Streams X through a device scratch in
 * chunks; the resident training shard is untouched. */
int sglm_predict_new(sglm_engine *h, const double *X, int64_t n, int64_t p, int64_t ldx,
                     const double *beta, const double *offset, const double *m, int family, int link,
                     int type, double *out);

/* ---- per-row diagnostics (R's hatvalues / residuals / cooks.distance / predict(se.fit = TRUE)) ----
 * Resident designs with p <= 256 on the fused / narrow path; procedural shards, wider designs and
 * SGLM_FORCE_WIDE return SGLM_EINVAL before any launch.  All rest on the row quadratic form
 * q_i = x_i' C x_i, C = inv(X'WX) (influence.hip).  Residuals are on the engine's count scale
 * (mu = unlink(eta, m)): divide binomial residuals by m for R's proportion scale. */
enum sglm_resid_type { SGLM_RESID_RESPONSE = 0, SGLM_RESID_WORKING = 1, SGLM_RESID_PEARSON = 2, SGLM_RESID_DEVIANCE = 3 };

/* Unscaled covariance inv(X'WX) at beta, col-major [p*p]: one IRLS pass at beta (collective over a
 * communicator, as sglm_irls_pass) and the fit's own solve rule; SGLM_ESINGULAR as the fit. */
int sglm_vcov(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, double *cov);

/* Per-row diagnostics of the resident rows at beta (computes sglm_vcov internally, so it is
 * collective too).  Any output may be NULL: hat [n_local] leverage h = w q; resid [n_local] of
 * resid_type (enum sglm_resid_type); cooks [n_local] = (r_P / (1 - h))^2 h / (dispersion p) with the
 * Pearson residual r_P whatever resid_type is; sum_hat: sum of h over the local rows, summed in a
 * fixed order (calls are run-to-run bitwise identical).  dispersion <= 0 is SGLM_EINVAL.  With hat,
 * cooks and sum_hat all NULL the quadratic forms are skipped.  A multi-device handle returns its
 * shards' rows concatenated in row order; with a communicator each rank gets its own rows against
 * the global C.  Gaussian / identity covers LM: w = 1, C = inv(X'X), dispersion = sigma^2. */
int sglm_influence(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, int resid_type,
                   double dispersion, double *hat, double *resid, double *cooks, double *sum_hat);

/* se.fit on the link scale for NEW rows: out[i] = sqrt(max(0, dispersion * x_i' cov x_i)), X
 * column-major n x p (ldx >= n, p <= 256), cov col-major [p*p] (sglm_vcov, or sglm_prelm.xtxi).
 * Streams X through sglm_predict_new's scratch; the resident shard is untouched. */
int sglm_predict_new_se(sglm_engine *h, const double *X, int64_t n, int64_t p, int64_t ldx,
                        const double *cov, double dispersion, double *out);

/* Kernel time of the last sglm_influence call on this handle (HIP events; a multi-device handle:
 * its slowest shard; -1 before any call). */
int sglm_get_influence_ms(sglm_engine *h, double *kernel_ms);

/* ---- heteroskedasticity-consistent ("sandwich") covariance: sandwich::vcovHC types HC0-HC3 ----
 * V = C M C with the bread C = inv(X'WX) at beta (sglm_vcov's matrix) and the meat
 * M = sum_i omega_i x_i x_i' over every row of every shard,
 *   omega_i = u_i^2 / (1 - h_i)^k,  u_i = w_i (y_i - mu_i) g'(mu_i),  h_i = w_i x_i' C x_i,
 * k = 0 (HC0, HC1), 1 (HC2), 2 (HC3); HC1 multiplies V by n / (n - p), n the global row count (rows of
 * prior weight 0 included, as vcovHC counts them; their omega is exactly 0).  The dispersion cancels:
 * V is the final covariance for every family.  Gaussian / identity without prior weights is White's
 * estimator for LM.  Same scope as the per-row diagnostics (resident, p <= 256; else SGLM_EINVAL before
 * any launch).  Reads the design three times: sglm_vcov's pass, the score-weight kernel (influence.hip)
 * and a Gram pass weighted by omega, reduced and all-reduced as every pass -- collective like sglm_vcov.
 * The resident data and a later fit are unchanged.  A non-finite M or V (a row with leverage 1 under
 * HC2 / HC3) is SGLM_EINVAL. */
enum sglm_hc_type { SGLM_HC0 = 0, SGLM_HC1 = 1, SGLM_HC2 = 2, SGLM_HC3 = 3 };
/* cov [p*p] col-major = C M C (x n/(n-p) for HC1), exactly symmetric; meat [p*p] col-major, may be NULL. */
int sglm_vcov_robust(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, int hc_type,
                     double *cov, double *meat);
/* Kernel times of the last sglm_vcov_robust call: score kernel, meat pass kernel (HIP events; a
 * multi-device handle: its slowest shard; -1 before any call). */
int sglm_get_sandwich_ms(sglm_engine *h, double *score_ms, double *meat_ms);

/* ---- cluster-robust covariance: sandwich::vcovCL(fit, cluster = ~id), Stata's vce(cluster id) ----
 * V = a C M C with the bread C of the sandwich above and the meat M = S'S, S [G x p] the cluster sums
 *   S[g, :] = sum_{i: id_i = g} u_i x_i      over every row of every shard,
 * u_i the signed score of the sandwich (exactly 0 where the prior weight is 0).  The adjustment a:
 * hc_type SGLM_HC0 none, SGLM_HC1 (n - 1) / (n - p) -- vcovCL's HC1, not vcovHC's n / (n - p); n the global
 * row count, rows of weight 0 included -- and with cadjust != 0 a further G / (G - 1).  HC1 with cadjust is
 * vcovCL's default and Stata's regress, vce(cluster); HC0 with cadjust Stata's glm / ML rule.  HC2 / HC3
 * (per-cluster leverage blocks) are SGLM_EINVAL.  Scope: that of sglm_vcov_robust.
 *
 * sglm_set_clusters declares the cluster of every resident row: dense codes 0 <= ids[i] < G, n_local = the
 * handle's resident rows (a multi-device handle: all its rows, in row order).  Local, not collective.  A
 * code without rows is allowed (its row of S is 0; it still counts in G).  ids = NULL clears.  A code out
 * of range, another n_local, or no data loaded: SGLM_EINVAL.  Any call that replaces the resident data
 * (sglm_set_data*, sglm_reserve, sglm_synth*) drops the clusters.  The engine cuts the rows into segments
 * (sglm_cluster_plan) and keeps nseg x p doubles for their sums: rows sorted by cluster, the usual panel
 * layout, give nseg ~ G + n / tile_rows, fully interleaved ids nseg = n -- SGLM_ENOMEM if that does not fit.
 *
 * sglm_vcov_cluster is collective, like sglm_vcov_robust: clusters may span shards and ranks, S is summed
 * over them through the handle's communicator -- G * p doubles per call (G rounded up to 32), beside the
 * p (p + 1) / 2 of the bread's pass -- and every rank then forms the same M.  Every rank must have declared
 * the same G (checked with one small all-reduce; else SGLM_EINVAL on every rank).  Also SGLM_EINVAL: no
 * clusters set, cadjust with G < 2, a non-finite M or V.  No floating-point atomics: results are run-to-run
 * bitwise identical, the order of every sum depends on (ids, n, p) only.  The resident data and a later fit
 * are unchanged.  cov [p*p] col-major, exactly symmetric; meat [p*p] col-major, may be NULL. */
int sglm_set_clusters(sglm_engine *h, const int32_t *ids, int64_t n_local, int32_t G);
int sglm_vcov_cluster(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, int hc_type, int cadjust,
                      double *cov, double *meat);
/* Kernel times of the last sglm_vcov_cluster call: score kernel, segment sums, combine, the meat's Gram pass
 * (HIP events; a multi-device handle: its slowest shard; -1 before any call). */
int sglm_get_cluster_ms(sglm_engine *h, double *score_ms, double *sum_ms, double *combine_ms, double *gram_ms);
/* The engine's segmentation of n rows with cluster codes ids (no device is touched): a segment is a
 * maximal run of consecutive rows with one code, additionally cut at every multiple of *tile_rows (a
 * compile-time constant), so nseg <= runs + ceil(n / tile_rows) and no segment crosses a tile.  seg_start
 * [nseg + 1] (the last entry is n) and seg_cluster [nseg]; either may be NULL (query *nseg first).  A code
 * outside [0, G) is SGLM_EINVAL. */
int sglm_cluster_plan(const int32_t *ids, int64_t n, int32_t G, int64_t *tile_rows, int64_t *nseg,
                      int64_t *seg_start, int32_t *seg_cluster);

/* ---- one-way fixed effects: the factor of sglm_set_clusters absorbed (fixest::feglm / fepois, Stata's
 * xtpoisson, fe / areg, alpaca::feglm) ----
 * The model eta_i = x_i' beta + alpha_{g(i)} + offset_i with one coefficient alpha_g per cluster, fitted by
 * the concentrated ("within") IRLS: at (beta, alpha) one ordinary pass with the effective offset
 * o*_i = offset_i + alpha_{g(i)} gives X'WX, X'Wz and the deviance; the group sums W_g = sum w_i,
 * t_g = sum w_i z_i, s_g = sum w_i x_i over every row of every shard and rank give
 *   A = X'WX - sum_g s_g s_g' / W_g,   b = X'Wz - sum_g s_g t_g / W_g,
 *   beta+ = inv(A) b (the fit's solve rule),   alpha_g+ = alpha_g + (t_g - s_g' beta+) / W_g.
 * By Frisch-Waugh-Lovell every iterate is that of sglm_fit_glm on [X | D], D the G dummy columns: start
 * (the initial-mode pass, alpha = 0), stop rule, dev_trace, iter, null_deviance, pearson and loglik are
 * sglm_fit_glm's; std_err = sqrt(diag(inv(A))), the beta block of the dummy fit's unscaled covariance.
 * X holds no intercept and no column that is constant within every group: such a column leaves a diagonal
 * element of A below 1e-10 of X'WX's and is SGLM_ESINGULAR.  Groups with W_g = 0 (no row, or only rows of
 * prior weight 0) contribute nothing, their alpha is NaN, and they do not count in G_eff;
 * df_residual = n - p - G_eff.  A group whose rows of positive prior weight all have y = 0 (poisson, negative
 * binomial, binomial) or all y = m (binomial) has no finite alpha: sglm_fit_glm_fe checks this on the device
 * before its first pass and returns SGLM_EINVAL naming how many such groups there are and the first.
 *
 * Scope: sglm_vcov_cluster's -- resident designs with p <= 256 on the fused / narrow path, else SGLM_EINVAL
 * before any launch; collective in the same way (group handles, RCCL, caller all-reduces), with one extra
 * all-reduce of G (p + 2) doubles (G rounded up to 32) per iteration beside the pass's; every rank ends
 * with bitwise the same beta and alpha.  No floating-point atomics: every order of summation depends on
 * (ids, n, p) only.  The resident data, the offset among them, and later calls of every other entry point
 * are unchanged.  SGLM_NEGBIN fits at the handle's theta (sglm_set_theta). */
typedef struct {
  int32_t G_eff;      /* groups with W_g > 0 at the solution */
  double df_residual; /* n - p - G_eff, n the global row count */
  double weights_ms, sum_ms, combine_ms, gram_ms; /* as sglm_get_fe_ms, of the last iteration */
} sglm_fe_info;
/* alpha [G] out; info may be NULL. */
int sglm_fit_glm_fe(sglm_engine *h, const sglm_glm_opts *opts, sglm_preglm *out, double *alpha, sglm_fe_info *info);
/* The test-level step at any (beta, alpha): A [p*p] col-major, b [p], group [G*(p+2)] = s [G x p] col-major |
 * t [G] | W [G], scalars [8] (the pass's); any output may be NULL.  beta == NULL selects opts' initial mode at
 * mu0 = mean(y) (alpha may then be NULL: zeros).  No uninformative-group check, no absorbed-column check. */
int sglm_fe_pass(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, const double *alpha, double *A,
                 double *b, double *group, double *scalars);
/* The covariance of beta at (beta, alpha).  cluster == 0: inv(A), the unscaled model-based covariance
 * (hc_type and cadjust are not read).  cluster != 0: V = a inv(A) M inv(A), clustered on the absorbed factor:
 * M = S'S, S_g = sum_{i in g} u_i x_i - U_g s_g / W_g with U_g = sum_{i in g} u_i (the second term vanishes
 * only at an exact solution) and u the signed score of sglm_vcov_cluster; a as sglm_vcov_cluster's with the
 * regressor count p replaced by p + G_eff: SGLM_HC0 none, SGLM_HC1 (n - 1) / (n - p - G_eff), cadjust a further
 * G / (G - 1); SGLM_HC2 / SGLM_HC3 are SGLM_EINVAL.  With this a, V is the beta block of sandwich::vcovCL on
 * the dummy fit.  An alpha that is NaN (a group without weight) is read as 0.  cov, meat [p*p] col-major;
 * meat may be NULL. */
int sglm_vcov_fe(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, const double *alpha, int cluster,
                 int hc_type, int cadjust, double *cov, double *meat);
/* Kernel times of the last fixed-effects step: the weights kernel, segment sums, combine, the Gram pass over
 * the group sums (HIP events; a multi-device handle: its slowest shard; -1 before any call). */
int sglm_get_fe_ms(sglm_engine *h, double *weights_ms, double *sum_ms, double *combine_ms, double *gram_ms);

/* ---- two-way fixed effects: a second absorbed factor beside the one of sglm_set_clusters (fixest::feglm /
 * fepois with two factors: unit x time panels, gravity models, worker x firm) ----
 * The model eta_i = x_i' beta + alpha_{g(i)} + gamma_{h(i)} + offset_i.  Factor 1 (G levels) is the factor of
 * sglm_set_clusters, factor 2 (H levels) that of sglm_set_fe2.  At (beta, alpha, gamma) one ordinary pass with
 * the effective offset o* = offset + alpha_g + gamma_h gives w, z, X'WX and X'Wz.  With M = [X | z], the level
 * sums S1 [G x (p+1)], S2 [H x (p+1)] of w M and the level weights W1, W2, the concentrated system is
 *   [A | b] = X'W[X | z] - S_X' Y,   Y = [a ; c] a solution of K Y = S, K = D'WD of the never formed dummies,
 * and Y comes from block Gauss-Seidel sweeps on the level coefficients (alternating projections):
 *   a_g <- (S1_g - sum_{i in g} w_i c_{h(i)}) / W1_g,   c_h <- (S2_h - sum_{i in h} w_i a_{g(i)}) / W2_h.
 * Then beta+ = inv(A) b, alpha+ = alpha + a_z - a_X beta+, gamma+ = gamma + c_z - c_X beta+.  No demeaned copy
 * of X is stored.  The sweeps of an iteration start from the Y of the one before (zero at the first) and stop
 * when the largest column-wise relative change of Y over one full sweep (max |change| / max |Y| per column
 * over both factors, then the maximum over the columns) is <= sweep_tol.  A factor-2 level that is the only
 * one of its component is an exact null direction: its c stays 0, and when every factor-2 level is such
 * (H = 1, or factor 2 a function of factor 1) one sweep is exact and is all that runs.
 *
 * K is singular with one null vector per connected component of the bipartite graph on the levels.  The
 * components are counted over all declared rows: a row of prior weight 0 still links its two levels.  Within
 * each component gamma of the lowest factor-2 code is 0 and alpha takes up the shift, so (alpha, gamma) are the
 * coefficients of the dummy fit on [X | D1 | D2 without those columns].  A level without weight has a = c = 0
 * and a NaN effect.  df_residual = n - p - (G_eff + H_eff - ncomp), fixest's count.
 *
 * sglm_set_fe2 declares the second factor: dense codes 0 <= ids2[i] < H, the rules of sglm_set_clusters (local,
 * NULL clears, dropped whenever the resident data are replaced).  It requires sglm_set_clusters; replacing or
 * clearing the clusters drops it.  The host sorts the rows by code (stable: a level's rows ascend), cuts each
 * level's rows into chunks of a compile-time length and keeps n_chunk <= H + ceil(n / chunk) rows of sums:
 * the memory does not depend on how the two factors interleave.
 *
 * Scope: sglm_fit_glm_fe's, narrowed to one device without a communicator (a multi-device handle or a handle
 * with a communicator is SGLM_EINVAL before any launch).  No floating-point atomics: every order of summation
 * depends on (ids1, ids2, n, p) only, results are run-to-run bitwise identical.  The resident data, the offset,
 * the clusters and every other entry point behave as before. */
typedef struct {
  double sweep_tol; /* 0: 1e-12 */
  int max_sweeps;   /* 0: 10000 (fixest's fixef.iter); reaching it is SGLM_EINVAL */
} sglm_fe2_opts;
typedef struct {
  int32_t G_eff, H_eff; /* levels with positive weight at the solution */
  int32_t ncomp;        /* connected components of the level graph over the declared rows */
  int32_t sweeps_last;  /* sweeps of the last iteration */
  int64_t sweeps_total;
  double df_residual;   /* n - p - (G_eff + H_eff - ncomp) */
  double weights_ms, sum1_ms, sum2_ms, sweep_ms, cross_ms; /* as sglm_get_fe2_ms, of the last iteration */
} sglm_fe2_info;
int sglm_set_fe2(sglm_engine *h, const int32_t *ids2, int64_t n_local, int32_t H);
/* The engine's plan for two factors (no device is touched): *chunk_len (a compile-time constant), *nchunk,
 * chunk_start [nchunk + 1] (positions in list), chunk_level [nchunk], list [n] (the rows ordered by factor-2
 * code, ascending within a code), *ncomp and comp_low [ncomp <= H] (each component's lowest factor-2 code,
 * ascending).  Any output may be NULL (query *nchunk first).  A code out of range is SGLM_EINVAL. */
int sglm_fe2_plan(const int32_t *ids1, const int32_t *ids2, int64_t n, int32_t G, int32_t H, int64_t *chunk_len,
                  int64_t *nchunk, int64_t *chunk_start, int32_t *chunk_level, int64_t *list, int32_t *ncomp,
                  int32_t *comp_low);
/* The fit: glm_drive over the two-way step, so start, stop rule, trace, null deviance, final statistics and
 * solve rule are sglm_fit_glm's.  alpha [G], gamma [H] out; fe2 and info may be NULL.  The absorbed-column
 * check of sglm_fit_glm_fe carries over (SGLM_ESINGULAR naming the column), and so does the uninformative-level
 * check, on both factors before the first pass (SGLM_EINVAL with a count and the first offender, naming the
 * factor). */
int sglm_fit_glm_fe2(sglm_engine *h, const sglm_glm_opts *opts, const sglm_fe2_opts *fe2, sglm_preglm *out,
                     double *alpha, double *gamma, sglm_fe2_info *info);
/* The test-level step at any (beta, alpha, gamma), the sweeps started from zero: A [p*p] col-major, b [p],
 * group1 [G*(p+2)] = S1_X [G x p] col-major | t1 | W1, group2 [H*(p+2)] likewise, Y [(G+H)*(p+1)] col-major
 * (a above c), scalars [8], *sweeps; any output may be NULL.  beta == NULL selects opts' initial mode (alpha and
 * gamma may then be NULL: zeros).  No uninformative-level check, no absorbed-column check. */
int sglm_fe2_pass(sglm_engine *h, const sglm_glm_opts *opts, const sglm_fe2_opts *fe2, const double *beta,
                  const double *alpha, const double *gamma, double *A, double *b, double *group1, double *group2,
                  double *Y, double *scalars, int *sweeps);
/* The covariance of beta at (beta, alpha, gamma).  cluster == 0: inv(A).  cluster != 0: clustered on factor 1,
 * V = a inv(A) M inv(A), M = S'S, S_g = sum_{i in g} u_i x_i - U_g a_g - sum_{i in g} u_i c_{h(i)} with a, c the
 * X columns of Y; a is sglm_vcov_fe's with p + G_eff replaced by p + G_eff + H_eff - ncomp.  SGLM_HC2 / SGLM_HC3
 * are SGLM_EINVAL.  A NaN effect is read as 0. */
int sglm_vcov_fe2(sglm_engine *h, const sglm_glm_opts *opts, const sglm_fe2_opts *fe2, const double *beta,
                  const double *alpha, const double *gamma, int cluster, int hc_type, int cadjust, double *cov,
                  double *meat);
/* Kernel times of the last two-way step, ms [5]: weights, factor-1 sums, factor-2 sums, sweeps, cross product
 * (HIP events; -1 before any call). */
int sglm_get_fe2_ms(sglm_engine *h, double *ms);

/* ---- GEE fits: the population-averaged GLM with an exchangeable working correlation over the cluster factor
 * of sglm_set_clusters (Liang & Zeger; geepack::geeglm(corstr = "exchangeable"), Stata xtgee, statsmodels GEE) ----
 * With d_i = sqrt(w_i) (w the IRLS working weight), R_g = (1 - rho) I + rho 11' has the inverse
 * (I - c_g 11') / (1 - rho), c_g = rho / (1 - rho + n_g rho), so one step's normal equations are
 *   A = (X'WX - sum_g c_g s_g s_g') / (1 - rho),   b = (X'Wz - sum_g c_g s_g t_g) / (1 - rho),
 *   s_g = sum_{i in g} d_i x_i,  t_g = sum_{i in g} d_i z_i
 * -- the fixed-effects downdate with sqrt(w) for w and c_g for 1 / W_g.  Per row e_i = d_i (y_i - mu_i) g'(mu_i)
 * (the Pearson residual up to the sign of g'), per group n_g (rows of positive prior weight), E_g = sum e_i,
 * Q_g = sum e_i^2; with N = sum n_g the moment estimates are (statsmodels / gee, ddof p)
 *   phi = sum Q_g / (N - p),   rho = [sum (E_g^2 - Q_g) / 2] / [(sum n_g (n_g - 1) / 2 - p) phi].
 * A step at beta: the pass at beta, the group sums (all-reduced), rho(beta) and phi(beta), A and b, the solve.
 * The initial-mode pass uses rho = 0.  SGLM_COR_INDEPENDENCE is rho = 0 throughout: every iterate is
 * sglm_fit_glm's, bitwise.  Scope, collectives and determinism: sglm_fit_glm_fe's.  SGLM_EINVAL before the first
 * pass without clusters, when sum n_g (n_g - 1) / 2 <= p or N <= p, and for a fixed rho with rho >= 1 or
 * 1 - rho + n_max rho <= 0; an estimated rho that leaves that range is SGLM_EINVAL naming the iteration. */
enum sglm_corstr { SGLM_COR_INDEPENDENCE = 0, SGLM_COR_EXCHANGEABLE = 1 };
typedef struct {
  int corstr;      /* enum sglm_corstr */
  int fix_rho;     /* != 0: use rho, do not estimate it (Stata corr(fixed)) */
  double rho;
} sglm_gee_opts;
typedef struct {
  double rho, phi; /* at the returned coefficients (a fixed rho: that value) */
  double N;        /* rows of positive prior weight */
  int32_t G_eff;   /* groups with such a row */
  int32_t n_max;   /* the largest n_g */
  double rows_ms, sum_ms, combine_ms, gram_ms; /* as sglm_get_gee_ms, of the last step */
} sglm_gee_info;
/* The fit: start, stop rule, dev_trace, iter, null_deviance, pearson and loglik are sglm_fit_glm's;
 * std_err = sqrt(diag(inv(A))) of the last solve, unscaled (the model-based one; sglm_vcov_gee has the robust
 * covariance).  gee NULL: exchangeable, rho estimated.  info may be NULL. */
int sglm_fit_glm_gee(sglm_engine *h, const sglm_glm_opts *opts, const sglm_gee_opts *gee, sglm_preglm *out,
                     sglm_gee_info *info);
/* The test-level step at any beta: A [p*p] col-major, b [p], group [G*(p+4)] = s [G x p] col-major | t | n | E | Q,
 * moments [5] = sum E_g^2, sum Q_g, sum n_g (n_g - 1) / 2, N, n_max, scalars [8], *rho_used (gee->rho with
 * fix_rho, else rho(beta)); any output may be NULL.  beta == NULL selects opts' initial mode with rho = 0. */
int sglm_gee_pass(sglm_engine *h, const sglm_glm_opts *opts, const sglm_gee_opts *gee, const double *beta, double *A,
                  double *b, double *group, double *moments, double *scalars, double *rho_used);
/* The covariance of beta at (beta, rho).  robust == 0: phi(beta) inv(A), the naive / model-based one.
 * robust != 0: inv(A) M inv(A), M = U'U, U_g = (sum_{i in g} d_i e_i x_i - c_g E_g s_g) / (1 - rho) (phi cancels);
 * cadjust: a further G / (G - 1).  Independence: rho is read as 0 and the robust covariance is
 * sglm_vcov_cluster(SGLM_HC0, cadjust).  meat [p*p] may be NULL (robust == 0: zeros). */
int sglm_vcov_gee(sglm_engine *h, const sglm_glm_opts *opts, const sglm_gee_opts *gee, const double *beta, double rho,
                  int robust, int cadjust, double *cov, double *meat);
/* Kernel times of the last GEE step, ms [4]: rows, segment sums, combine, the Gram pass over the group sums
 * (HIP events; -1 before any call). */
int sglm_get_gee_ms(sglm_engine *h, double *ms);

/* ---- Firth's bias-reduced fits (Firth 1993; logistf::logistf, brglm2::brglmFit(type = "AS_mean"), Stata
 * firthlogit): finite estimates under complete or quasi-complete separation, and the first-order bias of the ML
 * estimate removed ----
 * For binomial (logit, probit, cloglog) and poisson (log, identity, sqrt) -- the phi = 1 families -- on a resident
 * design with p <= 256.  The adjusted score at beta, on the engine's scales (binomial mu = m pi, prior weights,
 * offset), is
 *   g*(beta) = sum_i (u_i + h_i r_i / 2) x_i,  u_i = w_i (y_i - mu_i) g'(mu_i),  h_i = w_i x_i' inv(X'WX) x_i,
 *   r = (d2mu / deta2) / (dmu / deta): logit 1 - 2 pi, probit -eta, cloglog 1 - e^eta, log 1, sqrt 1 / eta, identity 0
 * -- for the canonical links the gradient of l(beta) + log det(X'WX) / 2 (the Jeffreys penalty).  A row of prior
 * weight 0 contributes exactly 0.  The fit iterates beta <- beta + inv(X'WX) g*(beta) from beta_start, or else
 * from sglm_fit_glm's first iterate (the initial pass of opts->init_mode and its solve), and stops with beta when
 * |inv(X'WX) g*|_1 < epsilon; a step after which |g*|_inf is not finite or larger than before is retried at half
 * its length, at most max_halvings times (then the last trial stands).  opts->tol and opts->max_iter are not read.
 * SGLM_EINVAL, before the handle is looked at: another family, epsilon <= 0 or not finite, maxit < 0; then a
 * procedural shard, p > 256 or SGLM_FORCE_WIDE.  Collective over a communicator, multi-device handles included;
 * two calls on the same shape and device give bitwise the same results (no floating-point atomics). */
typedef struct {
  double epsilon;   /* stop when the step's 1-norm is below it; R's brglmControl default 1e-8 */
  int maxit;        /* at most this many steps; 100 */
  int max_halvings; /* per step; 12 */
} sglm_firth_opts;
typedef struct {
  int iterations;      /* steps taken */
  int converged;       /* 0: maxit steps without meeting epsilon -- a returned status, not an error */
  int halvings;        /* over all steps */
  double deviance;     /* D at the returned coefficients */
  double pen_deviance; /* D* = D - log det(X'WX) */
  double logdet;       /* log det(X'WX) */
  double score_inf;    /* |g*|_inf */
  double sum_hat;      /* sum h_i (= p up to rounding) */
  double firth_ms;     /* kernel time of the last Firth pass, as sglm_get_firth_ms */
  double pass_ms;      /* kernel time of the last ordinary pass (the slowest shard) */
} sglm_firth_info;
/* Every returned quantity is evaluated at the returned coefficients: std_err = sqrt(diag(inv(X'WX))), deviance,
 * pearson, loglik (the unpenalised one); null_deviance and dev_trace as sglm_fit_glm (one entry per step);
 * iter = info->iterations.  firth_opts NULL: the defaults above; beta_start and info may be NULL. */
int sglm_fit_glm_firth(sglm_engine *h, const sglm_glm_opts *opts, const sglm_firth_opts *firth_opts,
                       const double *beta_start, sglm_preglm *out, sglm_firth_info *info);
/* The test-level pass at beta: A [p*p] col-major = X'WX, g [p] = g*, hat [n_local] = h (a multi-device handle:
 * every shard's rows, in row order), scalars [3] = deviance, log det A, sum h; any output may be NULL. */
int sglm_firth_pass(sglm_engine *h, const sglm_glm_opts *opts, const double *beta, double *A, double *g, double *hat,
                    double *scalars);
/* Kernel time of the last Firth pass, ms (HIP events; the slowest shard; -1 before any call). */
int sglm_get_firth_ms(sglm_engine *h, double *ms);

/* ---- Multinomial logit fits (softmax regression; nnet::multinom, Stata mlogit, statsmodels MNLogit) ----
 * A response with K unordered classes, 2 <= K <= 16, on a resident design with p <= 256 and q = (K - 1) p <= 1024.
 * y holds the class code of each row as a double, an integer in 0 .. K - 1; class 0 is the baseline.  B is
 * [p x (K - 1)] col-major, column j - 1 the coefficients of class j, so the parameter vector of length q is
 * class-major: index (j - 1) p + c.  Per row eta_0 = 0, eta_j = x' beta_j, pi = softmax(eta) (formed against
 * max(0, eta_1, ...); pi_0 is never 1 - sum); the deviance is D = -2 sum pw_i log pi_{y_i}, the log-likelihood
 * -D / 2, aic = D + 2 q, the null deviance -2 sum_k N_k log(N_k / N) over the weighted class counts N_k (the
 * intercept-only fit's closed form).  Score g = vec(X'R), R_ij = pw_i (1[y_i = j] - pi_ij); Hessian blocks
 * H_jj = X' diag(pw pi_j (1 - pi_j)) X, H_jk = -X' diag(pw pi_j pi_k) X.  Prior weights are supported; a row of
 * weight 0 contributes nothing and its y is not looked at.
 * The fit is Newton's method from B = 0 (nnet's start) or B_start: delta = solve(H, g) by the engine's solve rule;
 * B + t delta is tried at t = 1, 1/2, ... and accepted when D_new - D_old <= epsilon (|D_new| + 0.1), the search
 * abandoned (converged = 0) after max_halvings halvings; after an accepted step the fit stops when
 * |D_old - D_new| / (|D_new| + 0.1) < epsilon (R's glm.control rule), or at max_iter.
 * SGLM_EINVAL, before the handle is looked at: n_classes outside 2 .. 16, a null opts / B, epsilon <= 0 or not
 * finite, max_iter < 0, max_halvings < 0; then q > 1024, a procedural shard, p > 256 or SGLM_FORCE_WIDE, a handle
 * that carries trials m or an offset; then a y of positive weight that is no class code, a class without weight.
 * Collective over a communicator, multi-device handles included; two calls on the same shape and device give
 * bitwise the same results (no floating-point atomics). */
typedef struct {
  int n_classes;    /* K */
  double epsilon;   /* 1e-8 */
  int max_iter;     /* 100 */
  int max_halvings; /* per step; 12 */
} sglm_multinom_opts;
typedef struct {
  int iter, halvings, converged; /* accepted steps; halvings over all steps; 0: max_iter or an abandoned search */
  double deviance, null_deviance, loglik, aic, score_inf; /* at the returned coefficients; score_inf = |g|_inf */
  double class_weight[16];       /* N_k, zeros past K */
} sglm_multinom_info;
/* One evaluation at B: H [q*q] col-major, g [q], scalars3 = {deviance, sum pw, null deviance}, prob [n x K]
 * col-major (n: this handle's rows; a multi-device handle: every shard's, in row order); any output may be NULL.
 * H, g and prob all NULL: the deviance-only evaluation (nothing stored per row). */
int sglm_multinom_pass(sglm_engine *h, int n_classes, const double *B, double *H, double *g, double *scalars3,
                       double *prob);
/* B [q] out, std_err [q] = sqrt(diag(cov)), cov [q*q] = inv(H) at B; B_start, std_err, cov and info may be NULL. */
int sglm_fit_multinom(sglm_engine *h, const sglm_multinom_opts *opts, const double *B_start, double *B,
                      double *std_err, double *cov, sglm_multinom_info *info);
/* Kernel times of the last call, ms (HIP events; the slowest shard; -1 before any call): the row kernel of the last
 * evaluation, its second kernel X'R (0 at the fused shapes), and the weight kernels and Gram passes of the last
 * Hessian, each summed over the K (K - 1) / 2 block pairs. */
int sglm_get_multinom_ms(sglm_engine *h, double *rows_ms, double *xtr_ms, double *weight_ms, double *gram_ms);

int sglm_get_stats(sglm_engine *h, sglm_stats *out);
/* The kernel an engine would run a pass of an n x p shard with (enum sglm_pass_kernel, -1 on bad
 * arguments) and its name into name[namelen] -- the engine's own dispatch rule, for callers and CPU
 * tests.  fused_split: SGLM_FUSED_SPLIT's meaning (1 default threshold, 0 never K1r, N from P16 = N);
 * flags: 1 procedural shard, 2 forced wide path (SGLM_FORCE_WIDE).  No device is touched. */
int sglm_pass_kernel_for(int64_t n, int64_t p, int fused_split, int flags, int family, int link, char *name,
                         int64_t namelen);
int sglm_reset_stats(sglm_engine *h);

/* ---- external backend: the same IRLS driver over caller-computed partials ---------
 * Lets a host (or a test) run the engine's driver, solve and convergence logic over
 * partial sums produced elsewhere (e.g. a CPU shard).  pass() must write the packed
 * wire format: lower-triangular X'WX row-major (i>=j: i*(i+1)/2+j), then X'Wz [p], then
 * 8 scalars.  mode: 0 irls(beta), 1 init-single, 2 init-multiple, 3 lm-gram, 4 lm-resid. */
typedef struct {
  void *ctx;
  int64_t p;
  int (*local_sums)(void *ctx, double *out2 /* {sum y, n_local} */);
  int (*pass)(void *ctx, int mode, const double *beta, double mu0, double ybar, double *packed);
} sglm_backend;

/* fn: as sglm_set_comm's (the communicator thread unless SGLM_COMM_TIMEOUT_S=0).  SGLM_NEGBIN is
 * SGLM_EINVAL here: the pass callback carries no theta. */
int sglm_fit_glm_external(const sglm_backend *be, sglm_allreduce_fn fn, void *comm_ctx,
                          const sglm_glm_opts *opts, sglm_preglm *out);
int sglm_fit_lm_external(const sglm_backend *be, sglm_allreduce_fn fn, void *comm_ctx,
                         sglm_prelm *out);

/* ---- in-process communicator: N host threads in one process, one handle each ---------
 * (a JVM driver's thread pool over N single-device handles; the alternative to
 * sglm_create_multi).  Pass sglm_local_allreduce with sglm_local_comm_rank(c, r) as the
 * context of rank r to sglm_set_comm (on_device = 0) or sglm_fit_*_external.  The sum runs
 * in rank order, so every rank gets bitwise the same result. */
typedef struct sglm_local_comm sglm_local_comm;
int sglm_local_comm_create(int nranks, sglm_local_comm **out);
void sglm_local_comm_destroy(sglm_local_comm *c);
void *sglm_local_comm_rank(sglm_local_comm *c, int rank);
int sglm_local_allreduce(void *ctx, double *buf, int64_t count, void *stream, int on_device);

/* ---- model objects and printed summaries (host-side, C++) ---------------------- */
/* GLM.createObj (GLM.scala:59-88) derived fields. */
typedef struct {
  double df_residual, df_null, p_dispersion, aic;
} sglm_glm_derived;
int sglm_glm_create_obj(const sglm_preglm *pre, int64_t p, sglm_glm_derived *out);
/* GLM.summary text (GLM.scala:998-1025). xnames: p C strings. Returns bytes needed. */
int64_t sglm_glm_summary(const sglm_preglm *pre, int64_t p, const char *const *xnames,
                         const char *yname, const char *family, const char *link, char *buf,
                         int64_t buflen);
/* SummaryLM.print text (LM.scala:128-136). */
int64_t sglm_lm_summary(const sglm_prelm *pre, int64_t p, const char *const *xnames,
                        const char *yname, char *buf, int64_t buflen);
/* Helpers reproduced from utils.scala:146-169 and java.lang.Double.toString. */
double sglm_sig_digits(double num, int digits);
double sglm_round_digits(double num, int digits);
int64_t sglm_java_double_string(double x, char *buf, int64_t buflen);
/* 2*(1-Phi(|z|)) and 2*(1-T_df(|t|)) as used by the summaries. */
double sglm_pval_normal(double z);
double sglm_pval_t(double t, double df);

#ifdef __cplusplus
}
#endif
#endif /* SGLM_H */
