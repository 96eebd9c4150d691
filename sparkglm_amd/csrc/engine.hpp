// engine.hpp -- the HIP engine behind the C ABI: what its host translation units share.
// Private to engine.cpp, negbin.cpp, comm.cpp, wide_path.cpp, diagnostics.cpp, vcov_cluster.cpp, fe.cpp, fe2.cpp,
// gee.cpp, firth.cpp, multinom.cpp and ingest.cpp; never included by a .hip file.  The steps over the cluster factor (fixed effects, two-way,
// GEE) share one state per step kind (sglm_engine::GroupSums) and one frame (fe.cpp: group_sums_local,
// group_sums_finish, group_gram; StepBackend and drive_step_fit below).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/sglm.h"
#include "common.hpp"
#include "driver.hpp"
#include "kernels.hpp"

namespace sglm {

inline std::string hip_msg(hipError_t e, const char* what) {
  return std::string("HIP error in ") + what + ": " + hipGetErrorString(e);
}

#define HIPCHK(expr)                                  \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) {                           \
      sglm::set_error(sglm::hip_msg(_e, #expr));      \
      return SGLM_EHIP;                               \
    }                                                 \
  } while (0)

// Compensated (Neumaier) accumulation of the scalar partials (host side of rowmath.hpp's
// neumaier_add): the deviance sum decides the iteration count against an absolute 1e-6.
inline void neumaier_add(double& s, double& c, double x) {
  const double t = s + x;
  c += (std::fabs(s) >= std::fabs(x)) ? (s - t) + x : (x - t) + s;
  s = t;
}

inline double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// Cross-rank sums of the NS scalars (deviance, Pearson, loglik ingredients, ...) in rank order
// with compensation.  The all-reduce buffer carries, after the packed result, one block of
// `count` slots per rank in which only the owner's block is non-zero, so the all-reduce -- in
// whatever order RCCL or the caller adds -- delivers every rank's scalars exactly (x + 0 = x),
// and each rank then sums them itself, in rank order, Neumaier-compensated: the fit's deviance
// trajectory no longer depends on how many ranks the rows are spread over beyond ~1 ulp.  A plain
// all-reduce of the deviance adds up to G - 1 uncompensated roundings of up to half an ulp each
// (2.4e-7 at 1e9 rows, beside GLM.scala:452's absolute tol 1e-6).  The partition-order sum of the
// reference (GLM.scala:404-407) is the order used here; only the rounding is compensated.
inline void compensated_rank_sum(const double* blocks, int nranks, int64_t count, double* out) {
  for (int64_t k = 0; k < count; ++k) {
    double s = 0.0, c = 0.0;
    for (int r = 0; r < nranks; ++r) neumaier_add(s, c, blocks[(int64_t)r * count + k]);
    out[k] = s + c;
  }
}

// blocks (= partials of NS doubles) of the statistics pass and of the theta kernel; the LM device round trip and the
// host path alike.  At most 4096: ensure_workspace sizes the partials buffer for 4096 * NS doubles at least.
// (LM 1M x 20: 2048 blocks measured equal, 4096 +5 %: profiles/r04_lm_stats_blocks.txt)
inline int stats_blocks(int64_t rows) {
  return (int)std::min<int64_t>(4096, std::max<int64_t>(1024, rows / 131072));
}

// ---- communicators (comm.cpp) ----
double comm_timeout_ms_env();  // SGLM_COMM_TIMEOUT_S in ms (default 300 s; 0: unbounded)
std::string rank_str(int rank);
// The rank a caller-supplied communicator context stands for, when the engine can tell: the
// in-process communicator's rank contexts (sglm_local_comm_rank); -1 otherwise.
int known_rank(sglm_allreduce_fn fn, void* ctx);

// Wait, with a deadline, for the streams whose last work is a collective over `comms`.
int wait_collective(const std::vector<hipStream_t>& sts, std::vector<ncclComm_t*> comms, double timeout_ms, int rank,
                    const char* what, const std::vector<hipEvent_t>& starts = {});

// Caller-supplied all-reduce callbacks on a communicator thread owned by the handle, waited for
// with the deadline.
class CallbackRunner {
 public:
  explicit CallbackRunner(int device = -1) : device_(device) {}
  ~CallbackRunner();
  CallbackRunner(const CallbackRunner&) = delete;
  CallbackRunner& operator=(const CallbackRunner&) = delete;

  bool broken() const { return !broken_msg_.empty(); }
  // a timed-out device-buffer callback may still write its buffer: the owner must not free it
  bool leaked_device_buffer() const { return leaked_dev_; }
  void reset() {  // a new communicator
    broken_msg_.clear();
    leaked_dev_ = false;
  }
  int call(sglm_allreduce_fn fn, void* ctx, double* buf, int64_t count, void* stream, int on_device, double timeout_ms,
           int rank);

 private:
  struct State;
  void start();
  int device_;
  std::shared_ptr<State> st_;
  std::thread th_;
  std::string broken_msg_;
  bool leaked_dev_ = false;
};

struct Comm {
  int kind = 0;  // 0 none, 1 callback, 2 rccl
  sglm_allreduce_fn fn = nullptr;
  void* ctx = nullptr;
  int on_device = 0;
  ncclComm_t nccl = nullptr;
  int nranks = 1;
  int rank = -1;  // this handle's rank (RCCL, the in-process communicator, sglm_set_comm_rank); -1 unknown
  double ms = 0.0;
  double timeout_ms = 300e3;  // SGLM_COMM_TIMEOUT_S when the communicator was set (0: unbounded)
};

}  // namespace sglm

// One sglm_engine drives one HIP device (or, as a multi-device handle, routes to its shards'
// engines).  All state first; the member functions are defined in the file named above each group.
struct sglm_engine : public sglm::Backend {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  hipEvent_t evc = nullptr;  // end of the pass's device all-reduce (comm time = ev2 -> evc)
  hipEvent_t evpre = nullptr;  // before a small RCCL all-reduce: where its deadline starts
  int ncu = 256;

  // ---- resident shard ----
  int64_t n = 0, p = 0, n_pad = 0, nblocks = 0;
  double *dX = nullptr, *dy = nullptr, *dm = nullptr, *doff = nullptr, *dprior = nullptr, *deta = nullptr;
  // procedural shard (sglm_synth_procedural): X regenerated in the wide kernels, not stored
  sglm::ProcX procx{};

  // ---- pass workspace ----
  int P16 = 0, grid = 0;
  int64_t stride = 0;
  double *dbeta = nullptr, *dpart = nullptr, *dred = nullptr, *dsmall = nullptr;
  double *hbeta = nullptr, *hred = nullptr;
  double* hsmall = nullptr;  // pinned [64]: the final statistics' sums (stats)
  int64_t part_cap = 0, red_cap = 0, dsmall_cap = 0;
  sglm::Comm comm;
  std::unique_ptr<sglm::CallbackRunner> cbr;  // caller callbacks with a deadline (CallbackRunner)
  bool red_on_device = false;  // dred holds the all-reduced result of the last pass
  bool lp_stats = false;       // the last pass carried the final statistics (PassArgs::stats_in_pass)
  double stats_const = 0.0;    // the fit's initial-pass S_AUX2: constant part of in-pass Poisson / Gamma statistics
  int consts_family = -1;      // family whose initial pass produced stats_const on this data (-1: none)
  // deviance-only passes (Backend::pass_dev): the next enqueue_pass runs the row stage and the
  // scalar reduction but no Gram -- bitwise the scalars of the full pass.  SGLM_SPECULATE=0 off.
  bool dev_only = false, allow_spec = true;
  // narrow path (narrow.hip, p <= 64): barrier-free per-wave pipelines
  bool narrow = false;
  int fused_split = 1;  // SGLM_FUSED_SPLIT: 1 K1r from its default column-block count up, 0 never (K1), N >= 2 from P16 = N
  bool allow_lm_device = true;  // SGLM_LM_DEVICE=0: LM fits take the two host round trips (tests)
  bool lm_extras_pass = false;  // the next LM Gram pass also sums X'1 and y'y (lm_device, one pass)
  // negative binomial (negbin.cpp): theta of FAM_NEGBIN passes (0: never set; a group handle and its shards
  // hold the same value), and -- while sglm_fit_glm_nb's Poisson fit runs -- every IRLS pass stores eta (no
  // in-pass statistics), so that the theta kernel finds the fit's eta
  double theta = 0.0;
  bool want_eta = false;
  int64_t theta_launches = 0;  // theta_terms_kernel launches, and their kernel time (HIP events)
  double theta_ms = 0.0;
  hipEvent_t evt0 = nullptr, evt1 = nullptr;

  // ---- wide path (wide.hip; wide_path.cpp) ----
  bool wide = false, force_wide = false;
  // procedural shards in chunks (setup_proc_chunks): each pass generates C rows of X at a time
  // into an HBM scratch (the row kernel, while it forms eta) and runs the resident Gram kernels
  // over it -- X is generated once per pass instead of once per super-tile that reads it
  int64_t ch_rows = 0;  // rows per chunk (multiple of 32); 0: in-kernel generation (PROC kernels)
  int nch = 0;
  double *dxsc = nullptr, *dchunks = nullptr;
  bool allow_chunks = true;  // SGLM_PROC_CHUNKS=0 disables
  // SGLM_PROC_OVERLAP: chunks of an overlapped procedural pass (<= 1: one buffer, serial).  Round 2
  // measured it slower beside both Gram launches (250M x 512 logit: 1257 ms per pass serial, 1420 /
  // 1480 at 8 / 16 chunks -- the generator's integer + fp64 VALU slowed the Gram by 31-38 %).  Round 5
  // (VERDICT r4 item 6): gated to the off-diagonal launches (then SGLM_PROC_OV_GATE; the diagonal launch
  // goes first) and the generating row kernel at raised priority, 8 chunks: 1284.5 -> 1266.9 ms on one
  // box (ungated 1466.3, gated at normal priority 1285.7).  Round 5 then split the
  // generator off (proc_gen_kernel, 48 VGPRs) and let it start beside each chunk's diagonal launch,
  // which goes first; round 6 measured the other launch orders +4.5 % (generator held until the
  // diagonal launch is done) and +5.5 % (off-diagonal launch first) and retired them.
  int proc_ov_want = 8;
  bool proc_ov = false;      // double-buffered scratch, row kernels on st2 (as the resident overlap below)
  int64_t proc_ov_min = (int64_t)1 << 20;  // SGLM_PROC_OV_MIN: fewest rows per overlapped chunk
  int64_t proc_scratch_max = 0;  // SGLM_PROC_SCRATCH_MAX (GiB): cap on the procedural chunk scratch (0: none)
  // resident wide shards, overlapped passes: the rows are cut into nov chunks; the row kernel of
  // chunk c + 1 runs on a second stream (st2) beside the Gram kernels of chunk c, so only chunk 0's
  // row stage is exposed.  Each chunk is reduced into dchunks[c]; the chunks are summed in order.
  int ov_want = 16;                // SGLM_WIDE_OVERLAP: chunks per pass (<= 1: off)
  int64_t ov_min = (int64_t)1 << 16;  // SGLM_WIDE_OV_MIN: fewest rows per chunk (fewer chunks on small shards)
  int nov = 0;
  int64_t ov_rows = 0;             // rows per chunk (multiple of 32; the last chunk may be shorter)
  int rgrid_ov = 0;                // row-kernel grid of chunks >= 1 (one workgroup per CU)
  hipStream_t st2 = nullptr;
  // events of a chunked pass (nch or nov chunks, never both): [4 c .. 4 c + 3] row span and Gram span
  // of chunk c, [4 * chunks()] the st -> st2 fork
  std::vector<hipEvent_t> evchunk;
  double *dw = nullptr, *dwz = nullptr, *dgp = nullptr, *drp = nullptr;
  int64_t gp_cap = 0, rp_cap = 0, wstride = 0;
  int npan = 0, nst = 0, nslots = 0, ggrid = 0, rgrid = 0;
  int ggk[2] = {0, 0};  // persistent grid of the off-diagonal / diagonal Gram kernels
  sglm::WidePiece* dpieces[2] = {nullptr, nullptr};  // [0] off-diagonal, [1] diagonal super-tiles
  int* dwgb[2] = {nullptr, nullptr};
  int* dstr = nullptr;                          // [nst][2] partial slot range per super-tile
  bool has_sched[2] = {false, false};
  hipEvent_t evm = nullptr;
  rocblas_handle blas = nullptr;
  // wide-path device solve (SGLM_WIDE_SOLVE): 0 Cholesky (potrf / potrs / potri, the default),
  // 1 LU + explicit inverse (Breeze inv's algorithm: dgetrf + dgetri, utils.scala:103-105)
  int wide_lu = 0;

  // ---- ingest (sglm_reserve / sglm_set_rows; ingest.cpp): two pinned staging buffers, double-buffered ----
  static constexpr int64_t STAGE_DOUBLES = (int64_t)8 << 20;  // 64 MiB each
  double* hstage[2] = {nullptr, nullptr};
  hipEvent_t evstage[2] = {nullptr, nullptr};
  int stage_k = 0;
  int64_t rows_loaded = 0;  // rows covered by the blocks written since the shard was reserved
  std::vector<std::pair<int64_t, int64_t>> written;  // those blocks' row ranges, disjoint, sorted
  double load_ms = 0.0;     // host wall time in set_data / set_rows (staging + H2D)
  int64_t load_bytes = 0;

  // ---- scoring scratch: new rows (sglm_predict_new, sglm_predict_new_se), separate from the resident shard ----
  double *dxs = nullptr, *dvs = nullptr, *dms = nullptr, *dos = nullptr;
  int64_t xs_cap = 0, vs_cap = 0;

  // ---- diagnostics (influence.hip; diagnostics.cpp): leverage, residuals, Cook's distance, se.fit ----
  double *dct = nullptr, *hct = nullptr;          // C~ tiles: device / pinned [MAX_P16 (MAX_P16 + 1) / 2][INFL_TILE]
  double* dinf[3] = {nullptr, nullptr, nullptr};  // hat, resid, cooks of the resident rows, allocated when first asked for
  int64_t inf_cap[3] = {0, 0, 0};
  double* dhpart = nullptr;                       // per-workgroup sums of h, then their sum
  int64_t hpart_cap = 0;
  hipEvent_t evi0 = nullptr, evi1 = nullptr;
  double influence_ms = -1.0;                     // kernel time of the last influence call (-1: none yet)
  // sandwich covariance (sglm_vcov_robust): the score weights omega of the resident rows [n_pad], and
  // -- only while that call's meat pass runs -- the vector the pass takes for its prior weights
  double* domega = nullptr;
  int64_t omega_cap = 0;
  const double* meat_w = nullptr;
  double score_ms = -1.0, meat_ms = -1.0;         // kernel times of the last sglm_vcov_robust call (-1: none yet)
  // Firth's adjusted score (influence.hip firth_kernel; firth.cpp): per-workgroup partials [grid][p + 1], then
  // their sum [p + 1]; past the fused widths v goes through domega
  double* dgpart = nullptr;
  int64_t gpart_cap = 0;
  double firth_ms = -1.0;                         // kernel time of the last Firth pass (-1: none yet)

  // ---- multinomial logit (multinom.hip; multinom.cpp): sglm_fit_multinom / sglm_multinom_pass.  Allocated when
  // first asked for, released with the data: the probabilities P [K][n_pad], past the fused shapes R [K - 1][n_pad],
  // B [MN_MAX_Q], the workgroups' partials [grid][q + MN_NSC] and then their sum.  The Hessian's row weights go
  // through domega.
  double *dmnP = nullptr, *dmnR = nullptr, *dmnB = nullptr, *dmnpart = nullptr;
  int64_t mnP_cap = 0, mnR_cap = 0, mnpart_cap = 0;
  hipEvent_t evmn[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // rows start / end, X'R end, weights start / end
  bool mn_two = false;  // the last full evaluation ran multinom_xtr_kernel
  // kernel times of the last call: the row kernel, X'R (0: fused), the weight kernels and the Gram passes of the
  // last Hessian, each summed over its block pairs (-1: none yet)
  double mn_ms[4] = {-1.0, -1.0, -1.0, -1.0};

  // ---- cluster sums (cluster.hip; vcov_cluster.cpp): sglm_set_clusters / sglm_vcov_cluster ----
  int32_t cl_G = 0;                               // clusters declared for the resident rows (0: none set)
  int64_t cl_nseg = 0, cl_ntiles = 0;
  // one allocation: seg_start [nseg + 2] | tile_seg [ntiles + 1] | cl_seg [nseg] | per combine level
  // chunk_start [nchunk + 1], chunk_dst [nchunk] | seg_cluster [nseg]
  int64_t* dclidx = nullptr;
  const int64_t* seg_start() const { return dclidx; }
  const int64_t* tile_seg() const { return dclidx + cl_nseg + 2; }
  const int64_t* cl_seg() const { return tile_seg() + cl_ntiles + 1; }          // the segments ordered by cluster
  const int64_t* seg_cluster() const { return dclidx + cl_segcl_off; }          // as int64
  double* dR = nullptr;                           // segment sums [nseg][p]
  // the combine's levels (common.hpp CombineArgs): offsets into dclidx; rows of dP the level reads
  // (level 0 reads R through cl_seg) and writes
  struct CombineLevel {
    int64_t nchunk, start_off, dst_off, in_row, out_row;
  };
  std::vector<CombineLevel> cl_levels;
  double* dP = nullptr;                           // partial sums of the clusters of more than one chunk
  bool cl_S_stale = true;                         // S may hold sums of other ids: zero it before the combine
  // an engine on the same device whose design is S [G x p] (the combine kernel writes it there): its
  // tuned LM Gram pass forms the meat S'S.  Kept from call to call while G and p stay.
  sglm_engine* cl_inner = nullptr;
  hipEvent_t evcl[4] = {nullptr, nullptr, nullptr, nullptr};
  // kernel times of the last sglm_vcov_cluster call: score, segment sums, combine, Gram (-1: none yet)
  double cl_ms[4] = {-1.0, -1.0, -1.0, -1.0};

  // ---- fixed effects over the cluster factor (fe.hip; fe.cpp): sglm_fit_glm_fe / sglm_fe_pass / sglm_vcov_fe ----
  int64_t cl_prow = 0;                            // rows of dP (the combine's scratch)
  int64_t cl_segcl_off = 0;                       // offset in dclidx of seg_cluster [nseg]
  const double* off_override = nullptr;           // while set, the pass reads its offset here (o* = o + alpha_g)
  double *dfo = nullptr, *dalpha = nullptr;       // o* [n_pad]; alpha [G]
  // What a step over the cluster factor keeps on a shard, the fixed-effects and the GEE steps each their own (so
  // the results of one stay bitwise what they were beside the other): nq scalar columns follow the p of the sums.
  struct GroupSums {
    int nq;                                       // fe: 2 (t | W); gee: GEE_NQ (t | n | E | Q)
    double *q = nullptr, *qp = nullptr;           // per-segment scalar sums [nseg][nq]; their combine scratch [cl_prow][nq]
    // the group sums [G rounded up to 32][p + nq] (common.hpp GroupArgs), summed over shards and ranks in place;
    // g2: the step's sums kept while sglm_vcov_fe / sglm_vcov_gee form the score-weighted ones
    double *g = nullptr, *g2 = nullptr;
    bool stale = true;                            // g may hold other shards' sums: zero it before the combine
    hipEvent_t ev[2] = {nullptr, nullptr};        // the row kernel
    // kernel times of the last step: row kernel, segment sums, combine, Gram over the group sums (-1: none yet)
    double ms[4] = {-1.0, -1.0, -1.0, -1.0};
  };
  GroupSums fe{2};

  // ---- GEE with an exchangeable working correlation over the cluster factor (gee.hip; gee.cpp):
  // sglm_fit_glm_gee / sglm_gee_pass / sglm_vcov_gee.  dgm: moment partials [GEE_MOMENT_BLOCKS][NS] | out [NS]
  GroupSums gee{sglm::GEE_NQ};
  double* dgm = nullptr;

  // ---- two-way fixed effects (fe2.hip; fe2.cpp): the second factor of sglm_set_fe2, its row lists, the
  // level matrices of the sweeps and their scratch; dropped with the clusters ----
  struct Fe2State;
  Fe2State* fe2 = nullptr;
  // kernel times of the last two-way step: weights, factor-1 sums, factor-2 sums, sweeps, cross product
  double fe2_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

  // ---- group: single-process multi-device handle (sglm_create_multi): the shards' engines; this
  // handle then only routes and reduces (one process owns all GPUs, as SURVEY 8(b) asks) ----
  std::vector<sglm_engine*> subs;
  std::vector<sglm_engine*> self{this};  // shards() of a single-device handle
  std::vector<int64_t> sub_lo;       // first global row of each shard
  std::vector<ncclComm_t> gcomms;    // ncclCommInitAll over distinct devices (else host sums)
  bool group_aborted = false;        // a group all-reduce missed its deadline (wait_collective)
  int64_t g_n = 0;                   // group: total rows

  // ---- stats ----
  int64_t passes = 0, dev_passes = 0;
  double pass_ms = 0.0, reduce_ms = 0.0, last_pass_ms = 0.0, last_reduce_ms = 0.0, row_ms = 0.0, gram_ms = 0.0;
  // LM fits keep their own last timing (pass_untimed): another pass kind in between must not be booked as LM time
  double lm_last_pass_ms = -1.0, lm_last_reduce_ms = 0.0;
  int64_t lm_device_fits = 0;
  int64_t lm_onepass_fits = 0;  // of those, fits whose statistics came from the Gram pass's sums
  int last_kernel = SGLM_KERNEL_NONE;  // the kernel of the last pass (enum sglm_pass_kernel) and its name
  char last_kernel_name[64] = "";

  // ---- accessors ----
  bool group() const { return !subs.empty(); }
  // the engines that hold this handle's rows: a group's shards, else the handle itself
  const std::vector<sglm_engine*>& shards() const { return group() ? subs : self; }
  int64_t ncols() const override { return group() ? subs[0]->p : p; }
  bool pass_has_stats() const override { return group() ? subs[0]->lp_stats : lp_stats; }
  int npart() const override { return group() ? (int)subs.size() : comm.nranks; }
  bool has_dev_pass() const override { return allow_spec; }
  bool comm_on_device() const { return comm.kind == 2 || (comm.kind == 1 && comm.on_device); }
  // scalars summed across ranks through rank blocks (compensated_rank_sum): needs >1 rank and a
  // known own rank; otherwise the communicator's plain sum
  bool gather_ranks() const { return comm.kind != 0 && comm.nranks > 1 && comm.rank >= 0 && comm.rank < comm.nranks; }
  // chunks of a chunked wide pass (resident overlapped, or procedural), 0 if the pass is not chunked
  int chunks() const { return nov > 0 ? nov : nch; }
  // chunks whose row kernels run beside the Gram (resident or procedural), 0 if none
  int ov_chunks() const { return nov > 1 ? nov : (proc_ov ? nch : 0); }

  // ---- engine.cpp: lifetime, workspace, passes ----
  ~sglm_engine() override;
  void free_data();
  void release();
  int alloc_data(int64_t n_, int64_t p_, bool has_m, bool has_off, bool has_prior, bool proc = false);
  int ensure_workspace();
  int ensure_red_len(int64_t len);  // dred / hred / dbeta / hbeta hold at least len doubles
  int ensure_small(int64_t count);
  // hipMalloc that reports SGLM_ENOMEM and names the buffer
  static int dev_alloc(double** ptr, size_t bytes, const char* what);
  // a grow-only device buffer of doubles: at least `need` afterwards, the old contents not kept
  static int grow(double*& ptr, int64_t& cap, int64_t need, const char* what);
  static void dev_free(std::initializer_list<double**> ptrs);  // hipFree and null each
  int global_sums(double* out2) override;
  int pass_dev(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override;
  int pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed) override;
  void finish_scalars(int mode, int family, double* s);
  int pass_timing();
  void pass_untimed();
  int enqueue_pass(int mode, const double* beta, double mu0, double ybar, int family, int link, bool timed = true);
  void note_kernel(int family, int link);
  int group_pass(int mode, const double* beta, double mu0, double ybar, int family, int link, double* packed);
  int lm_device(double* packed, double* dev_coefs, double* s, bool& done) override;
  int stats(int mode, const double* beta, double mu0, double ybar, int family, int link, double* s) override;

  // ---- negbin.cpp: theta on the handle, the theta terms ----
  int theta_check(int family) const;  // SGLM_EINVAL: a FAM_NEGBIN call on a handle without theta
  // {score, info, loglik (if asked), sum w (y/mu - 1)^2, sum w} at theta over the eta of the last pass,
  // all-reduced (shards in order / rank blocks, compensated)
  int theta_terms(int link, double th, bool loglik, double* out5);
  int theta_terms_local(int link, double th, bool loglik, double* s);

  // ---- comm.cpp: the communicator ----
  sglm::CallbackRunner& runner();
  void leak_comm_buffers();
  int call_comm(double* buf, int64_t count, int on_device);
  int allreduce_device(double* dbuf, int64_t count, bool after_pass = false);
  int allreduce_host(double* hbuf, int64_t count);
  int allreduce_small(double* h, int64_t count);
  int stage_rank_block(int r, int nr);

  // ---- wide_path.cpp: schedules, workspace, the wide pass, the device solver ----
  void free_schedule();
  bool banded_kind(int S, int64_t nb, int G) const;
  int build_wide_schedule();
  int ensure_chunk_events(int nc);
  int ensure_wide_workspace();
  int setup_proc_chunks();
  double* rowpart(int c) const;
  int launch_grams(sglm::WideGramArgs& g, bool diag_first);
  int enqueue_wide(int mode, bool has_beta, double mu0, double ybar, int family, int link);
  int wide_timing(float k1);
  std::unique_ptr<sglm::SolverIface> make_solver(int64_t pp) override;
  int blas_handle();

  // ---- ingest.cpp: host rows in, scores of new rows out ----
  int ensure_staging();
  int h2d_block(double* dst, int64_t dld, const double* src, int64_t sld, int64_t rows, int64_t cols);
  int set_rows(int64_t row0, int64_t nr, const double* X, int64_t ldx, const double* yv, const double* mv,
               const double* ov, const double* pv);
  int check_loaded() const;
  int ensure_new_rows(int64_t pp, int64_t chunk);
  int predict_new(const double* X, int64_t nn, int64_t pp, int64_t ldx, const double* beta, const double* off,
                  const double* mv, int family, int link, int type, double* out);

  // ---- diagnostics.cpp ----
  void free_influence();
  int upload_cov(const double* cov, int64_t pp);
  // One launch of the row kernel (influence.hip) in `mode` (enum InflMode) over the resident shard at beta, on the
  // stream between evi0 and evi1.  a: the mode's own fields (outputs, hc_k, resid_type, dispersion, gpart); the
  // shard's are filled here.  cov: the global C (null: need_q = 0, nothing uploaded).  to_omega: a.out is domega
  // feeding a later pass -- grown here, zeros on its padding rows.  An empty shard launches nothing (both events
  // are recorded).  rows_grid: the launch's workgroups, by which a caller sizes the partials it asks for;
  // rows_sync: the stream drained, ms = the kernel time of the launch.
  int rows_enqueue(int mode, const double* beta, const double* cov, int family, int link, sglm::InflArgs a,
                   bool to_omega = false);
  int rows_grid(int mode) const;
  int rows_sync(double* ms);
  int influence_local(const double* beta, const double* cov, int family, int link, int rtype, double disp, double* hat,
                      double* resid, double* cooks, double* sum_hat);
  int score_local(const double* beta, const double* cov, int family, int link, int k);
  // g [p + 1] = the adjusted score g* | sum of h of this shard's rows at beta against cov (the global C); hat [n]
  // or null
  int firth_local(const double* beta, const double* cov, int family, int link, double* g, double* hat);
  int predict_new_se(const double* X, int64_t nn, int64_t pp, int64_t ldx, const double* cov, double disp, double* out);

  // ---- multinom.cpp ----
  void free_multinom();
  // The rows of this shard at B [(K - 1) p] in `mode` (common.hpp MnMode) and the fixed-order sum of the
  // workgroups' partials, enqueued on the stream; then out [nscore + MN_NSC] = the score (MN_FULL) | the scalars,
  // prob (or null) [K] columns ldp apart = P of this shard's rows, the stream drained, the kernel times taken
  int multinom_enqueue(int K, const double* B, int mode);
  int multinom_collect(int K, int mode, double* out, double* prob, int64_t ldp);
  // domega = the row weights of the Hessian's block pair (j, k) from P, enqueued
  int multinom_weight_local(int K, int j, int k);

  // ---- vcov_cluster.cpp ----
  void free_clusters(bool inner_too);
  int set_clusters_local(const int32_t* ids, int64_t nl, int32_t G);
  int uscore_local(const double* beta, int family, int link);
  int ensure_cl_inner();  // the internal engine whose design is [G x p]
  int cluster_sums_local();
  // the combine tree over the cluster factor's segments: the unit sums R [nseg][ncol] into S (scratch P)
  int combine_clusters(const double* R, double* P, int ncol, double* S, int64_t ldS, hipEvent_t e0 = nullptr,
                       hipEvent_t e1 = nullptr);
  int cluster_sync();
  int64_t cluster_len() const { return cl_inner->n_pad * p; }  // doubles of S, padding included

  // ---- fe.cpp: the one-way fixed effects, and the group sums they share with the GEE fits ----
  void free_fe();
  int fe_prepare();
  // effects [L] to dst on this device; a NaN (a level without weight) is read as 0; null: zeros
  int set_effects(double* dst, const double* src, int64_t L);
  int fe_offset_local();
  // va, vb: where the kernel stores the two per-row values it sums (common.hpp SegRowArgs), or null
  int fe_sums_local(int kind, int mode, int family, int link, double mu0, double* va = nullptr, double* vb = nullptr);
  int fe_sync();
  int64_t group_len(const GroupSums& gs) const { return cl_inner->n_pad * (p + gs.nq); }  // doubles of g, padding included
  void free_group(GroupSums& gs);
  int group_prepare(GroupSums& gs);  // the buffers of a step on this shard (kept until the clusters or the data change)
  // The row values of a kind and this shard's group sums into gs.g, enqueued on the stream: the row kernel (`launch`
  // of launch_fe_weights / launch_gee_rows, reading the offset `off`), with `rows` the segment sums of u x (u:
  // domega) through the combine tree into the first p columns, then the kernel's nq per-segment scalars through
  // the same tree into the columns after them (evcl[2] to evcl[3] spans both trees)
  using RowLaunch = hipError_t (*)(const sglm::SegRowArgs&, int, hipStream_t, hipEvent_t, hipEvent_t);
  int group_sums_local(GroupSums& gs, RowLaunch launch, bool rows, int kind, int mode, int family, int link, double mu0,
                       const double* off, double* va, double* vb);
  int keep_group_sums(GroupSums& gs);  // g into g2 (allocated when first asked for), enqueued

  // ---- fe2.cpp ----
  void free_fe2();

  // ---- gee.cpp ----
  void free_gee();
  int gee_prepare();
  // the row values of `kind` (common.hpp GeeKind) and this shard's group sums into gee.g: enqueued on the stream
  int gee_sums_local(int kind, int mode, int family, int link, double mu0);
};

namespace sglm {

inline int check_handle(sglm_engine* h) {
  if (!h) {
    set_error("requirement failed: null engine handle");
    return SGLM_EINVAL;
  }
  return SGLM_OK;
}

// ---- vcov_cluster.cpp: what the fixed-effects fits share with the cluster-robust covariance ----
// The number of clusters every shard (and every rank: one small all-reduce) declared; SGLM_EINVAL
// on every rank when they differ or none are set.
int cluster_count(sglm_engine* h, int32_t* G);
// A buffer of `len` doubles that every shard holds (buf(shard): the cluster sums S, cl_inner->dX and cluster_len();
// a step's group sums, GroupSums::g and group_len()) summed in place over the handle's shards or ranks; every rank
// (a group: shard 0) ends with bitwise the same sums.
int sum_cluster_scores(sglm_engine* h, const std::function<double*(sglm_engine*)>& buf, int64_t len);
// The combine tree's plan.  An open range is a destination row of S and the positions [lo, hi) it owns in the
// level's input (ascending, contiguous).  A range is cut into chunks of CLUSTER_CHUNK positions.  One chunk: it is
// summed into S and the range is done.  Several: each is summed into a row of the scratch, and those rows are
// the range at the next level.  Appends per level chunk_start [nchunk + 1], chunk_dst [nchunk] to idx and fills
// levels; returns the rows of the scratch.
struct CombineRange {
  int64_t dst, lo, hi;
};
int64_t plan_combine(std::vector<CombineRange> cur, std::vector<int64_t>& idx,
                     std::vector<sglm_engine::CombineLevel>& levels);
// The tree's launches on s's stream: unit sums R [.][ncol] (level 0 reads them through idx0, null: as they lie),
// scratch P, into S; `base` is the device copy of the planner's idx.  e0 / e1: recorded at the start of the
// first level and the end of the last (no level: no launch, neither is recorded).
int combine_levels(sglm_engine* s, const std::vector<sglm_engine::CombineLevel>& levels, const int64_t* base,
                   const int64_t* idx0, const double* R, double* P, int ncol, double* S, int64_t ldS,
                   hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// The refusals of a clustered covariance: hc_type; cadjust once G is known
int check_cluster_hc(int hc_type);
int check_cadjust(int cadjust, int32_t G);
// cov = f C M C with f from HC1's (nrows - 1) / (nrows - p - absorbed) and cadjust's G / (G - 1); the meat
// copied out.  `at` closes the refusal of a covariance that is not finite ("beta", "(beta, alpha)").
int clustered_finish(int hc_type, double nrows, int64_t p, int64_t absorbed, int32_t G, int cadjust,
                     const std::vector<double>& C, const std::vector<double>& M, const char* at, double* cov,
                     double* meat);

// ---- fe.cpp: what the two-way fixed-effects fits (fe2.cpp) and the GEE fits (gee.cpp) share with the one-way ones ----
// what every entry point of a step requires, before any launch, and the buffers of the step (`prepare`, on every
// shard); `needs` opens the refusal of a handle off the fused / narrow path
int fe_check(sglm_engine* h, const sglm_glm_opts* opts, int32_t* G, const char* needs = "a fixed-effects fit needs",
             int (sglm_engine::*prepare)() = &sglm_engine::fe_prepare);
// which of a shard's sums a step works on: &sglm_engine::fe or &sglm_engine::gee
using GroupSumsOf = sglm_engine::GroupSums sglm_engine::*;
// after every shard's local sums of a step were enqueued (group_sums_local): synchronise, take the kernel times
// (GroupSums::ms, the slowest shard; rows: the segment sums and the combine too), sum over shards and ranks
int group_sums_finish(sglm_engine* h, GroupSumsOf gs, bool rows);
// The group rows of shard 0 scaled into its internal engine (`scale`: launch_fe_scale / launch_gee_scale, at rho;
// meat: the score-weighted sums in g beside the step's in g2) and that engine's LM Gram pass: packed [packed_len(p)]
int group_gram(sglm_engine* h, GroupSumsOf gs, hipError_t (*scale)(const GroupArgs&, hipStream_t), bool meat, double rho,
               double* packed);
// A fit's Backend whose pass is a step over the handle (fixed effects, two-way, GEE): everything else is the handle's
struct StepBackend : public Backend {
  sglm_engine* h;
  explicit StepBackend(sglm_engine* handle) : h(handle) {}
  int64_t ncols() const override { return h->ncols(); }
  int npart() const override { return h->npart(); }
  int global_sums(double* out2) override { return h->global_sums(out2); }
  int stats(int mode, const double* beta, double mu0, double ybar, int family, int link, double* s) override {
    return h->stats(mode, beta, mu0, ybar, family, link, s);
  }
  std::unique_ptr<SolverIface> make_solver(int64_t p) override { return h->make_solver(p); }
};
// glm_drive over such a backend; the solves' time and path into the handle
int drive_step_fit(StepBackend& be, const sglm_glm_opts& opts, sglm_preglm* out);
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
// the group sums of `kind` (common.hpp FeKind) over the cluster factor into shard 0's fe.g, synchronised;
// va, vb as sglm_engine::fe_sums_local
int fe_group_sums(sglm_engine* h, int kind, int mode, int family, int link, double mu0, double* va = nullptr,
                  double* vb = nullptr);
// SGLM_ESINGULAR naming column j, which the fixed effects absorb
int absorbed_error(int64_t j);
constexpr double FE_ABSORBED_RATIO = 1e-10;  // A_jj below this part of X'WX_jj: fixest's collin.tol
// (mode, mu0) of a step entry point: at beta, or at the initial mean when beta is null (collective)
int fe_step_mode(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, int* mode, double* mu0);
// a step's packed = lower tri A | b | scalars into the outputs that are wanted
void fe_unpack_step(const double* packed, int64_t p, double* A, double* b, double* scalars);
// the covariance of a call without clustering: the bread itself, a zero meat
int fe_plain_cov(const std::vector<double>& C, double* cov, double* meat);
// columns [col0, col0 + ncol) of a col-major level buffer on s's device, the first L rows of each, to the host
int download_cols(sglm_engine* s, const double* buf, int64_t ld, int64_t L, int64_t col0, int64_t ncol, double* out);
// levels of positive weight W; the effect (where given) of every other level becomes NaN
int32_t count_weighted(const std::vector<double>& W, double* effects);
// ab = a [L] | b [L], the check's two sums per level: levels of which exactly one is 0 (both 0: no row of
// positive weight) have no finite effect -- their count and the first of them
std::pair<int64_t, int64_t> uninformative_levels(const std::vector<double>& ab);

// ---- diagnostics.cpp: what the covariance estimators share ----
// inv(X'WX) at beta (collective over a communicator), the bread of both sandwich estimators
int vcov_impl(sglm_engine* h, const sglm_glm_opts* opts, const double* beta, double* cov);
// The bread C [p x p] = inv(A) of a pass's or a step's packed A by the fit's solve rule, log det A where asked for
// (the solve's time and path into the handle); `singular`: the message of a singular A
int bread(sglm_engine* h, double* packed, const char* singular, double* C, double* logdet = nullptr);
// a kernel time of a call over the handle's shards (ms(shard)): the slowest shard's
template <class F>
double slowest_shard(const sglm_engine* h, F ms) {
  double v = ms(h->shards()[0]);
  for (const sglm_engine* s : h->shards()) v = std::max(v, ms(s));
  return v;
}
// SGLM_EINVAL unless every shard is a resident design on the fused / narrow path
int require_fused_or_narrow(const sglm_engine* h, const char* what);
// While it lives, the passes of the handle's shards weight their rows by domega: the sandwich's score weights
// (sglm_vcov_robust), the multinomial Hessian's block weights (multinom.cpp).
struct MeatPassScope {
  sglm_engine* h;
  explicit MeatPassScope(sglm_engine* handle) : h(handle) {
    for (sglm_engine* s : h->shards()) s->meat_w = s->domega;
  }
  ~MeatPassScope() {
    for (sglm_engine* s : h->shards()) s->meat_w = nullptr;
  }
};
// cov = f (C M C + (C M C)') / 2, exactly symmetric (col-major p x p, on the host); false: M or cov is not finite
bool sandwich_product(const std::vector<double>& C, const std::vector<double>& M, int64_t p, double f, double* cov);

// The handle holds a complete design: every reserved row written (or generated).
inline int check_ready(sglm_engine* h) {
  for (sglm_engine* s : h->shards())
    if (int rc = s->check_loaded()) return rc;
  return SGLM_OK;
}

}  // namespace sglm
