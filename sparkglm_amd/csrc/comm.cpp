// comm.cpp -- the engine's communicators: bounded waits on the per-iteration all-reduce, caller
// callbacks with a deadline, the engine's all-reduce helpers, the communicator setters of the C ABI
// (sglm_set_comm*) and the in-process communicator (sglm_local_comm).
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "engine.hpp"

using namespace sglm;

// ---- in-process communicator: N host threads, one handle each (a JVM driver's thread pool) ----
// Every rank's call blocks until all N have arrived; the last to arrive sums the N buffers in
// rank order (deterministic, independent of arrival order) and writes the sum into all of them.
struct sglm_local_comm {
  int nranks = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t generation = 0;
  std::vector<double*> bufs;
  int64_t count = -1;
  bool failed = false;  // this round: a rank passed another count
  bool result = false;  // the last completed round failed (read by its waiters only)
  double timeout_ms = 0.0;  // SGLM_COMM_TIMEOUT_S, read once by sglm_local_comm_create
  struct Rank {
    sglm_local_comm* c;
    int rank;
  };
  std::vector<Rank> ranks;
};

namespace sglm {

// ---- bounded waits on the per-iteration all-reduce (utils.scala:110-126's treeReduce seam) ----
// A rank that dies or stalls must not hang the others until an outside time limit: every wait on
// a collective has a deadline, SGLM_COMM_TIMEOUT_S seconds (default 300; 0 = unbounded), read when
// the communicator is set.  On expiry (or an asynchronous RCCL error) the call returns SGLM_ECOMM
// naming the rank and what it waited for, and the communicator is unusable from then on.
double comm_timeout_ms_env() {
  const char* e = std::getenv("SGLM_COMM_TIMEOUT_S");
  if (!e || !*e) return 300e3;
  const double s = std::atof(e);
  return s > 0.0 ? s * 1e3 : 0.0;
}

std::string rank_str(int rank) { return rank >= 0 ? "rank " + std::to_string(rank) : "this rank"; }

int known_rank(sglm_allreduce_fn fn, void* ctx) {
  if (fn == &sglm_local_allreduce && ctx) return static_cast<sglm_local_comm::Rank*>(ctx)->rank;
  return -1;
}

// Wait for the streams whose last work is a collective over `comms` (the engine's RCCL
// communicator, or a multi-device handle's ncclCommInitAll group): poll hipStreamQuery and every
// communicator's asynchronous error until the streams drain or the deadline passes.  On a remote
// error or expiry the communicators are aborted (ncclCommAbort makes their kernels exit) and
// nulled, and SGLM_ECOMM is returned -- never a silent hang.  `starts`: events recorded on those
// streams just before the collective (this rank's own pass done); the deadline counts from the
// moment all of them have completed, so it bounds the wait for the peers, never this rank's own
// pass kernels (a long pass on a large shard cannot expire it).
int wait_collective(const std::vector<hipStream_t>& sts, std::vector<ncclComm_t*> comms, double timeout_ms,
                    int rank, const char* what, const std::vector<hipEvent_t>& starts) {
  for (hipEvent_t ev : starts) {  // this rank's pass kernels: no deadline (they need no peer)
    hipError_t e;
    while ((e = hipEventQuery(ev)) == hipErrorNotReady) std::this_thread::yield();
    if (e != hipSuccess) {
      set_error(hip_msg(e, "hipEventQuery (the pass before the all-reduce)"));
      return SGLM_EHIP;
    }
  }
  const double t0 = now_ms();
  std::vector<char> done(sts.size(), 0);
  size_t left = sts.size();
  auto abort_all = [&](const std::string& why) {
    for (ncclComm_t* c : comms)
      if (*c) {
        (void)ncclCommAbort(*c);
        *c = nullptr;
      }
    set_error(why);
    return SGLM_ECOMM;
  };
  for (uint64_t it = 0; left > 0; ++it) {
    for (size_t i = 0; i < sts.size(); ++i) {
      if (done[i]) continue;
      const hipError_t e = hipStreamQuery(sts[i]);
      if (e == hipSuccess) {
        done[i] = 1;
        --left;
      } else if (e != hipErrorNotReady) {
        set_error(hip_msg(e, "hipStreamQuery (wait on the all-reduce)"));
        return SGLM_EHIP;
      }
    }
    if (left == 0) break;
    if ((it & 255) == 255) {
      for (ncclComm_t* c : comms) {
        ncclResult_t ae = ncclSuccess;
        if (*c && ncclCommGetAsyncError(*c, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress)
          return abort_all(std::string("RCCL asynchronous error on ") + rank_str(rank) + " during " + what + ": " +
                           ncclGetErrorString(ae) + "; communicator aborted");
      }
      if (timeout_ms > 0.0 && now_ms() - t0 > timeout_ms)
        return abort_all(rank_str(rank) + ": " + what + " did not complete within SGLM_COMM_TIMEOUT_S = " +
                         std::to_string(timeout_ms * 1e-3) + " s (a peer rank died, stalled or never joined); "
                         "communicator aborted");
    }
    std::this_thread::yield();
  }
  return SGLM_OK;
}

// Caller-supplied all-reduce callbacks (sglm_set_comm, sglm_fit_*_external) run on a communicator
// thread owned by the handle -- one thread for the handle's life, with the handle's device
// current -- while the calling thread waits with the deadline.  A callback that never returns is
// abandoned (its thread detached with its own copy of a host buffer) and the handle's communicator
// is marked broken.  sglm_local_allreduce is bounded by itself and runs inline.
struct CallbackRunner::State {
  std::mutex mu;
  std::condition_variable cv;
  bool has_job = false, done = false, stop = false;
  sglm_allreduce_fn fn = nullptr;
  void* ctx = nullptr;
  double* buf = nullptr;
  int64_t count = 0;
  void* stream = nullptr;
  int on_device = 0, rc = 0;
  std::vector<double> host;
};

CallbackRunner::~CallbackRunner() {
  if (!st_) return;
  {
    std::lock_guard<std::mutex> lk(st_->mu);
    st_->stop = true;
  }
  st_->cv.notify_all();
  if (th_.joinable()) th_.join();
}

int CallbackRunner::call(sglm_allreduce_fn fn, void* ctx, double* buf, int64_t count, void* stream, int on_device,
                         double timeout_ms, int rank) {
  if (broken()) {
    set_error(broken_msg_);
    return SGLM_ECOMM;
  }
  if (timeout_ms <= 0.0 || fn == &sglm_local_allreduce) {
    if (fn(ctx, buf, count, stream, on_device) != 0) {
      set_error(fn == &sglm_local_allreduce
                    ? "in-process all-reduce failed on " + rank_str(rank) +
                          " (ranks passed different lengths, or a rank did not arrive within SGLM_COMM_TIMEOUT_S)"
                    : "caller all-reduce failed on " + rank_str(rank));
      return SGLM_ECOMM;
    }
    return SGLM_OK;
  }
  start();
  std::unique_lock<std::mutex> lk(st_->mu);
  st_->fn = fn;
  st_->ctx = ctx;
  st_->count = count;
  st_->stream = stream;
  st_->on_device = on_device;
  if (on_device) {
    st_->buf = buf;
  } else {
    st_->host.assign(buf, buf + count);
    st_->buf = st_->host.data();
  }
  st_->done = false;
  st_->has_job = true;
  st_->cv.notify_all();
  const bool ok = st_->cv.wait_for(lk, std::chrono::duration<double, std::milli>(timeout_ms), [&] { return st_->done; });
  if (!ok) {
    lk.unlock();
    broken_msg_ = rank_str(rank) + ": the caller all-reduce did not return within SGLM_COMM_TIMEOUT_S = " +
                  std::to_string(timeout_ms * 1e-3) + " s (a peer rank died, stalled or never joined); the "
                  "communicator is broken -- set a new one";
    leaked_dev_ = on_device != 0;
    th_.detach();  // the thread keeps its state (and the host copy) alive by itself
    st_.reset();
    set_error(broken_msg_);
    return SGLM_ECOMM;
  }
  if (!on_device) std::memcpy(buf, st_->host.data(), sizeof(double) * (size_t)count);
  if (st_->rc != 0) {
    set_error("caller all-reduce failed on " + rank_str(rank));
    return SGLM_ECOMM;
  }
  return SGLM_OK;
}

void CallbackRunner::start() {
  if (st_) return;
  st_ = std::make_shared<State>();
  std::shared_ptr<State> s = st_;
  const int dev = device_;
  th_ = std::thread([s, dev] {
    if (dev >= 0) (void)hipSetDevice(dev);
    std::unique_lock<std::mutex> lk(s->mu);
    for (;;) {
      s->cv.wait(lk, [&] { return s->has_job || s->stop; });
      if (s->stop) return;
      s->has_job = false;
      lk.unlock();
      const int rc = s->fn(s->ctx, s->buf, s->count, s->stream, s->on_device);
      lk.lock();
      s->rc = rc;
      s->done = true;
      s->cv.notify_all();
    }
  });
}

}  // namespace sglm

// ---- the engine's communicator helpers ----
CallbackRunner& sglm_engine::runner() {
  if (!cbr) cbr.reset(new CallbackRunner(device));
  return *cbr;
}

// a caller callback abandoned at its deadline may still write the device buffer it was given:
// those buffers are leaked, never freed under it
void sglm_engine::leak_comm_buffers() {
  dred = dsmall = nullptr;
  red_cap = dsmall_cap = 0;
}

int sglm_engine::call_comm(double* buf, int64_t count, int on_device) {
  const int rc = runner().call(comm.fn, comm.ctx, buf, count, (void*)st, on_device, comm.timeout_ms, comm.rank);
  if (rc && runner().leaked_device_buffer()) leak_comm_buffers();
  return rc;
}

// after_pass: dbuf is the pass just enqueued (ev2 marks its end on st); the RCCL time is then
// ev2 -> evc on the device (this rank's wait for the others included), not the host wall time
// of a synchronize that would also cover the pass kernels.
int sglm_engine::allreduce_device(double* dbuf, int64_t count, bool after_pass) {
  if (comm.kind == 2) {
    if (!comm.nccl) {
      set_error(rank_str(comm.rank) + ": the RCCL communicator was aborted by an earlier failure; set a new one");
      return SGLM_ECOMM;
    }
    const double t0 = now_ms();
    // the deadline starts when everything this rank queued before the collective is done: the pass
    // (ev2, recorded at its end) or, for the small all-reduces, whatever precedes them on st
    if (!after_pass) {
      if (!evpre) HIPCHK(hipEventCreateWithFlags(&evpre, hipEventDisableTiming));
      HIPCHK(hipEventRecord(evpre, st));
    }
    ncclResult_t r = ncclAllReduce(dbuf, dbuf, (size_t)count, ncclFloat64, ncclSum, comm.nccl, st);
    if (r != ncclSuccess) {
      set_error(std::string("RCCL ncclAllReduce on ") + rank_str(comm.rank) + ": " + ncclGetErrorString(r));
      return SGLM_ECOMM;
    }
    if (after_pass) HIPCHK(hipEventRecord(evc, st));
    if (int rc = wait_collective({st}, {&comm.nccl}, comm.timeout_ms, comm.rank, "ncclAllReduce",
                                 {after_pass ? ev2 : evpre}))
      return rc;
    if (after_pass) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev2, evc));
      comm.ms += ms;
    } else {
      comm.ms += now_ms() - t0;
    }
  } else if (comm.kind == 1 && comm.on_device) {
    HIPCHK(hipStreamSynchronize(st));
    const double t0 = now_ms();
    if (int rc = call_comm(dbuf, count, 1)) return rc;
    comm.ms += now_ms() - t0;
  }
  return SGLM_OK;
}

int sglm_engine::allreduce_host(double* hbuf, int64_t count) {
  if (comm.kind == 1 && !comm.on_device) {
    const double t0 = now_ms();
    if (int rc = call_comm(hbuf, count, 0)) return rc;
    comm.ms += now_ms() - t0;
  }
  return SGLM_OK;
}

// all-reduce a small host vector (count scalar sums) through whichever path the communicator uses
int sglm_engine::allreduce_small(double* h, int64_t count) {
  if (comm.kind == 0) return SGLM_OK;
  std::vector<double> blocks;
  double* b = h;
  int64_t len = count;
  if (gather_ranks()) {  // this rank's values in its own block, zeros elsewhere
    blocks.assign((size_t)(count * comm.nranks), 0.0);
    std::memcpy(blocks.data() + (int64_t)comm.rank * count, h, sizeof(double) * count);
    b = blocks.data();
    len = count * comm.nranks;
  }
  if (comm_on_device()) {
    if (int rc = ensure_small(len)) return rc;
    HIPCHK(hipMemcpyAsync(dsmall, b, sizeof(double) * len, hipMemcpyHostToDevice, st));
    int rc = allreduce_device(dsmall, len);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(b, dsmall, sizeof(double) * len, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  } else if (int rc = allreduce_host(b, len)) {
    return rc;
  }
  if (b != h) compensated_rank_sum(b, comm.nranks, count, h);
  return SGLM_OK;
}

// this shard's scalars into rank block `r` of the nr blocks after the packed result, zeros in the
// others (device buffer, on st)
int sglm_engine::stage_rank_block(int r, int nr) {
  const int64_t plen = packed_len(p), sc = tri_count(p) + p;
  HIPCHK(hipMemsetAsync(dred + plen, 0, sizeof(double) * (size_t)(NS * nr), st));
  HIPCHK(hipMemcpyAsync(dred + plen + (int64_t)r * NS, dred + sc, sizeof(double) * NS, hipMemcpyDeviceToDevice, st));
  return SGLM_OK;
}

static int no_group(sglm_engine* h, const char* what) {
  if (!h->group()) return SGLM_OK;
  set_error(std::string("requirement failed: ") + what +
            " joins one device to other processes; a multi-device handle already reduces over its devices");
  return SGLM_EINVAL;
}

extern "C" {

int sglm_set_comm(sglm_engine* h, sglm_allreduce_fn fn, void* ctx, int on_device) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = no_group(h, "sglm_set_comm")) return rc;
  h->comm.kind = fn ? 1 : 0;
  h->comm.fn = fn;
  h->comm.ctx = ctx;
  h->comm.on_device = on_device;
  h->comm.nranks = 1;
  h->comm.rank = known_rank(fn, ctx);
  h->comm.timeout_ms = comm_timeout_ms_env();
  if (h->cbr) h->cbr->reset();
  if (fn) {  // count the ranks joined by the caller's communicator
    double one[1] = {1.0};
    if (on_device) {
      HIPCHK(hipSetDevice(h->device));
      if (int rc = h->ensure_small(64)) return rc;
      HIPCHK(hipMemcpy(h->dsmall, one, sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipStreamSynchronize(h->st));
      if (int rc = h->call_comm(h->dsmall, 1, 1)) return rc;
      HIPCHK(hipStreamSynchronize(h->st));
      HIPCHK(hipMemcpy(one, h->dsmall, sizeof(double), hipMemcpyDeviceToHost));
    } else if (int rc = h->call_comm(one, 1, 0)) {
      return rc;
    }
    h->comm.nranks = (int)std::lround(one[0]);
  }
  return SGLM_OK;
}

int sglm_rccl_unique_id(void* out128) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) {
    set_error(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    return SGLM_ECOMM;
  }
  std::memcpy(out128, &id, sizeof id);
  return SGLM_OK;
}

int sglm_set_comm_rccl(sglm_engine* h, int nranks, int rank, const void* unique_id128) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = no_group(h, "sglm_set_comm_rccl")) return rc;
  if (nranks < 1 || rank < 0 || rank >= nranks || !unique_id128) {
    set_error("requirement failed: 0 <= rank < nranks, unique id");
    return SGLM_EINVAL;
  }
  HIPCHK(hipSetDevice(h->device));
  if (h->comm.nccl) (void)ncclCommDestroy(h->comm.nccl);
  ncclUniqueId id;
  std::memcpy(&id, unique_id128, sizeof id);
  ncclResult_t r = ncclCommInitRank(&h->comm.nccl, nranks, id, rank);
  if (r != ncclSuccess) {
    h->comm.nccl = nullptr;
    set_error(std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    return SGLM_ECOMM;
  }
  h->comm.kind = 2;
  h->comm.nranks = nranks;
  h->comm.rank = rank;
  h->comm.timeout_ms = comm_timeout_ms_env();
  if (int rc = h->ensure_small(64)) return rc;
  return SGLM_OK;
}

int sglm_set_comm_rank(sglm_engine* h, int rank) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = no_group(h, "sglm_set_comm_rank")) return rc;
  if (h->comm.kind == 0) {  // no communicator: no other rank to wait for
    set_error("requirement failed: a communicator joined first (sglm_set_comm), 0 <= rank < its rank count");
    return SGLM_EINVAL;
  }
  // Collective: with a rank the scalars travel in per-rank blocks, which lengthens every later
  // all-reduce, so every rank must opt in -- with distinct ranks -- or the ranks would post
  // collectives of different sizes.  Every rank joins one plain all-reduce of [bad | one-hot of
  // its rank], a rank whose own check fails with bad = 1 (never returning before the collective,
  // which would leave the others waiting in it): the ranks are valid and distinct iff bad sums to
  // 0 and every one-hot slot to exactly 1.
  HIPCHK(hipSetDevice(h->device));
  h->comm.rank = -1;
  const int nr = h->comm.nranks;
  const bool local_ok = rank >= 0 && rank < nr;
  std::vector<double> chk((size_t)nr + 1, 0.0);
  chk[0] = local_ok ? 0.0 : 1.0;
  if (local_ok) chk[(size_t)rank + 1] = 1.0;
  if (int rc = h->allreduce_small(chk.data(), (int64_t)chk.size())) return rc;
  bool ok = chk[0] == 0.0;
  for (int k = 0; k < nr; ++k) ok = ok && chk[(size_t)k + 1] == 1.0;
  if (!ok) {
    set_error("requirement failed: sglm_set_comm_rank must be called by every rank of the communicator, each with "
              "its own distinct rank in [0, " + std::to_string(h->comm.nranks) + ")");
    return SGLM_EINVAL;
  }
  h->comm.rank = rank;
  return SGLM_OK;
}

int sglm_local_comm_create(int nranks, sglm_local_comm** out) {
  if (!out || nranks < 1) {
    set_error("requirement failed: nranks >= 1, out");
    return SGLM_EINVAL;
  }
  auto* c = new sglm_local_comm();
  c->nranks = nranks;
  c->timeout_ms = comm_timeout_ms_env();  // once, here: no getenv on the rank threads' all-reduces
  c->bufs.assign((size_t)nranks, nullptr);
  for (int r = 0; r < nranks; ++r) c->ranks.push_back({c, r});
  *out = c;
  return SGLM_OK;
}

void sglm_local_comm_destroy(sglm_local_comm* c) { delete c; }

void* sglm_local_comm_rank(sglm_local_comm* c, int rank) {
  if (!c || rank < 0 || rank >= c->nranks) return nullptr;
  return &c->ranks[(size_t)rank];
}

int sglm_local_allreduce(void* ctx, double* buf, int64_t count, void* stream, int on_device) {
  (void)stream;
  auto* rk = static_cast<sglm_local_comm::Rank*>(ctx);
  if (!rk || on_device) return 1;  // host buffers only
  sglm_local_comm* c = rk->c;
  std::unique_lock<std::mutex> lk(c->mu);
  const uint64_t gen = c->generation;
  if (c->arrived == 0) {
    c->count = count;
    c->failed = false;
  } else if (count != c->count) {
    c->failed = true;
  }
  c->bufs[(size_t)rk->rank] = buf;
  if (++c->arrived == c->nranks) {
    if (!c->failed) {
      std::vector<double> sum(c->bufs[0], c->bufs[0] + count);
      for (int r = 1; r < c->nranks; ++r)
        for (int64_t k = 0; k < count; ++k) sum[(size_t)k] += c->bufs[(size_t)r][k];
      for (int r = 0; r < c->nranks; ++r) std::memcpy(c->bufs[(size_t)r], sum.data(), sizeof(double) * count);
    }
    c->result = c->failed;
    c->arrived = 0;
    ++c->generation;
    c->cv.notify_all();
  } else {
    // bounded (SGLM_COMM_TIMEOUT_S): a rank that never arrives fails the round for everyone
    // instead of leaving the others blocked; the one timing out withdraws its buffer
    const double tmo = c->timeout_ms;
    auto arrived = [&] { return c->generation != gen; };
    if (tmo > 0.0) {
      if (!c->cv.wait_for(lk, std::chrono::duration<double, std::milli>(tmo), arrived)) {
        c->bufs[(size_t)rk->rank] = nullptr;
        --c->arrived;
        c->failed = true;
        return 1;
      }
    } else {
      c->cv.wait(lk, arrived);
    }
  }
  return c->result ? 1 : 0;
}

}  // extern "C"
