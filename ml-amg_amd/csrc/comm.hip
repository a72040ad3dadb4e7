// Multi-GPU transport: communicators and halo exchange. The partitioned V-cycle executor that
// runs on it is dhier.hip; comm.hpp is what the two share.
//
// A communicator is one rank of a group, over one of three transports: RCCL (one process per
// GPU; mlamg_comm_create), the in-process loopback below (several ranks on one device, for
// tests) or a null transport that skips every exchange (timing only). All of them offer grouped
// send/recv of doubles and a sum all-reduce with RCCL's semantics (xgroup_begin .. xgroup_end,
// xallreduce_sum). A halo holds, for a row-partitioned vector x_ext = [owned | ghosts], the
// neighbour ranks, the owned entries each of them needs (packed by k_pack into a send buffer)
// and where each neighbour's entries land among the ghosts; halo_exchange_impl is the pack
// followed by one grouped exchange, and the two halves are exposed separately so the executor
// can run the exchange on a second stream while interior rows compute.
#include "comm.hpp"

#include <rccl/rccl.h>

#include <chrono>
#include <functional>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

// In-process transport for testing the executor with several ranks on ONE device (RCCL refuses
// two ranks on one GPU): every rank is a host thread with its own stream; a send posts (buffer,
// ready event) into a shared mailbox, the receiver orders its stream after the ready event and
// copies device-to-device, and the sender's stream is then ordered after that copy (so it cannot
// overwrite its send buffer early). Same message order and grouping semantics as the RCCL calls
// it stands in for; never used by a communicator made with mlamg_comm_create.
struct LoopPost {
  const double* p = nullptr;
  size_t n = 0;
  hipEvent_t ready = nullptr;
  hipEvent_t done = nullptr;
  bool consumed = false;
  ~LoopPost() {
    if (ready) (void)hipEventDestroy(ready);
    if (done) (void)hipEventDestroy(done);
  }
};

struct LoopRound {  // one all-reduce: every rank's (buffer, ready), then (copied) events
  std::vector<const double*> buf;
  std::vector<hipEvent_t> ready, copied;
  int posted = 0, finished = 0, left = 0;
};

struct mlamg_loop_group {
  int W = 1;
  std::mutex mu;
  std::condition_variable cv;
  std::map<std::tuple<int, int, uint64_t>, std::shared_ptr<LoopPost>> box;
  std::vector<uint64_t> send_seq, recv_seq;  // [src * W + dst]
  std::map<uint64_t, LoopRound> rounds;
  int members = 0;
};

struct mlamg_comm {
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  mlamg_loop_group* loop = nullptr;  // in-process test transport instead of RCCL
  bool null_transport = false;       // timing only: exchanges skipped (results are NOT valid)
  struct Recv {
    double* buf;
    size_t n;
    int peer;
  };
  std::vector<std::shared_ptr<LoopPost>> sends;  // posted in the open group
  std::vector<Recv> recvs;                       // completed at group end
  uint64_t ar_seq = 0;
  double* ar_stage = nullptr;
  size_t ar_cap = 0;
};

struct mlamg_halo {
  mlamg_comm* c = nullptr;
  int64_t n_own = 0, n_ghost = 0;
  std::vector<int> nbr;
  std::vector<int64_t> send_off, send_cnt, recv_off, recv_cnt;
  int32_t* send_idx = nullptr;  // device, concatenated per neighbour
  double* send_buf = nullptr;   // device
  int64_t n_send = 0;
};

#define MLAMG_NCCL(call)                                                            \
  do {                                                                              \
    ncclResult_t _r = (call);                                                       \
    if (_r != ncclSuccess) {                                                        \
      ::mlamg::set_error(std::string(#call) + " failed: " + ncclGetErrorString(_r)); \
      return MLAMG_ENCCL;                                                           \
    }                                                                               \
  } while (0)

namespace mlamg {

constexpr auto kLoopTimeout = std::chrono::seconds(120);

static int loop_wait(mlamg_loop_group* g, std::unique_lock<std::mutex>& lk,
                     const std::function<bool()>& ready, const char* what) {
  if (!g->cv.wait_for(lk, kLoopTimeout, ready)) {
    set_error(std::string("loopback transport: timed out waiting for ") + what);
    return MLAMG_ENCCL;
  }
  return MLAMG_OK;
}

int xgroup_begin(mlamg_comm* c) {
  if (c->null_transport) return MLAMG_OK;
  if (!c->loop) MLAMG_NCCL(ncclGroupStart());
  return MLAMG_OK;
}

int xsend(mlamg_comm* c, const double* buf, size_t n, int peer, hipStream_t s) {
  if (c->null_transport) return MLAMG_OK;
  if (!c->loop) {
    MLAMG_NCCL(ncclSend(buf, n, ncclFloat64, peer, c->comm, s));
    return MLAMG_OK;
  }
  auto post = std::make_shared<LoopPost>();
  post->p = buf;
  post->n = n;
  MLAMG_HIP(hipEventCreateWithFlags(&post->ready, hipEventDisableTiming));
  MLAMG_HIP(hipEventRecord(post->ready, s));
  mlamg_loop_group* g = c->loop;
  {
    std::lock_guard<std::mutex> lk(g->mu);
    const uint64_t seq = g->send_seq[c->rank * g->W + peer]++;
    g->box[std::make_tuple(c->rank, peer, seq)] = post;
  }
  g->cv.notify_all();
  c->sends.push_back(post);
  return MLAMG_OK;
}

int xrecv(mlamg_comm* c, double* buf, size_t n, int peer, hipStream_t s) {
  if (c->null_transport) return MLAMG_OK;
  if (!c->loop) {
    MLAMG_NCCL(ncclRecv(buf, n, ncclFloat64, peer, c->comm, s));
    return MLAMG_OK;
  }
  c->recvs.push_back({buf, n, peer});
  return MLAMG_OK;
}

int xgroup_end(mlamg_comm* c, hipStream_t s) {
  if (c->null_transport) return MLAMG_OK;
  if (!c->loop) {
    MLAMG_NCCL(ncclGroupEnd());
    return MLAMG_OK;
  }
  mlamg_loop_group* g = c->loop;
  std::vector<mlamg_comm::Recv> recvs;
  recvs.swap(c->recvs);
  std::vector<std::shared_ptr<LoopPost>> sends;
  sends.swap(c->sends);
  for (const auto& r : recvs) {
    std::shared_ptr<LoopPost> post;
    {
      std::unique_lock<std::mutex> lk(g->mu);
      const auto key = std::make_tuple(r.peer, c->rank, g->recv_seq[r.peer * g->W + c->rank]);
      MLAMG_TRY(loop_wait(g, lk, [&] { return g->box.count(key) != 0; }, "a matching send"));
      post = g->box[key];
      g->box.erase(key);
      ++g->recv_seq[r.peer * g->W + c->rank];
    }
    MLAMG_REQUIRE(post->n == r.n, "loopback transport: send/recv sizes differ");
    MLAMG_HIP(hipStreamWaitEvent(s, post->ready, 0));
    if (r.n) MLAMG_HIP(hipMemcpyAsync(r.buf, post->p, sizeof(double) * r.n, hipMemcpyDeviceToDevice, s));
    MLAMG_HIP(hipEventCreateWithFlags(&post->done, hipEventDisableTiming));
    MLAMG_HIP(hipEventRecord(post->done, s));
    {
      std::lock_guard<std::mutex> lk(g->mu);
      post->consumed = true;
    }
    g->cv.notify_all();
  }
  for (const auto& p : sends) {
    {
      std::unique_lock<std::mutex> lk(g->mu);
      MLAMG_TRY(loop_wait(g, lk, [&] { return p->consumed; }, "the receiver of a send"));
    }
    MLAMG_HIP(hipStreamWaitEvent(s, p->done, 0));
  }
  return MLAMG_OK;
}

__global__ void k_loop_sum(const double* __restrict__ stage, int W, int64_t n,
                           double* __restrict__ out) {
  const int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  double t = stage[i];
  for (int r = 1; r < W; ++r) t += stage[(int64_t)r * n + i];
  out[i] = t;
}

int xallreduce_sum(mlamg_comm* c, double* buf, size_t n, hipStream_t s) {
  if (c->null_transport) return MLAMG_OK;
  if (!c->loop) {
    MLAMG_NCCL(ncclAllReduce(buf, buf, n, ncclFloat64, ncclSum, c->comm, s));
    return MLAMG_OK;
  }
  mlamg_loop_group* g = c->loop;
  const int W = g->W;
  if (c->ar_cap < (size_t)W * n) {
    MLAMG_HIP(hipStreamSynchronize(s));
    if (c->ar_stage) (void)hipFree(c->ar_stage);
    c->ar_stage = nullptr;
    MLAMG_HIP(hipMalloc(&c->ar_stage, sizeof(double) * std::max<size_t>((size_t)W * n, 1)));
    c->ar_cap = (size_t)W * n;
  }
  const uint64_t round = c->ar_seq++;
  hipEvent_t ready = nullptr, copied = nullptr;
  MLAMG_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
  MLAMG_HIP(hipEventRecord(ready, s));
  std::vector<const double*> bufs;
  std::vector<hipEvent_t> readies;
  {
    std::unique_lock<std::mutex> lk(g->mu);
    LoopRound& R = g->rounds[round];
    if (R.buf.empty()) {
      R.buf.assign(W, nullptr);
      R.ready.assign(W, nullptr);
      R.copied.assign(W, nullptr);
    }
    R.buf[c->rank] = buf;
    R.ready[c->rank] = ready;
    ++R.posted;
    g->cv.notify_all();
    MLAMG_TRY(loop_wait(g, lk, [&] { return g->rounds[round].posted == W; }, "all-reduce peers"));
    bufs = g->rounds[round].buf;
    readies = g->rounds[round].ready;
  }
  // every rank's buffer, in rank order, into this rank's staging area
  for (int r = 0; r < W; ++r) {
    MLAMG_HIP(hipStreamWaitEvent(s, readies[r], 0));
    if (n) MLAMG_HIP(hipMemcpyAsync(c->ar_stage + (size_t)r * n, bufs[r], sizeof(double) * n,
                                    hipMemcpyDeviceToDevice, s));
  }
  MLAMG_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
  MLAMG_HIP(hipEventRecord(copied, s));
  std::vector<hipEvent_t> copies;
  {
    std::unique_lock<std::mutex> lk(g->mu);
    LoopRound& R = g->rounds[round];
    R.copied[c->rank] = copied;
    ++R.finished;
    g->cv.notify_all();
    MLAMG_TRY(loop_wait(g, lk, [&] { return g->rounds[round].finished == W; }, "all-reduce copies"));
    copies = g->rounds[round].copied;
  }
  // nobody reads this rank's buffer any more once every copy is done: overwrite it
  for (int r = 0; r < W; ++r) MLAMG_HIP(hipStreamWaitEvent(s, copies[r], 0));
  if (n) {
    hipLaunchKernelGGL(k_loop_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       c->ar_stage, W, (int64_t)n, buf);
    MLAMG_HIP(hipGetLastError());
  }
  {
    std::lock_guard<std::mutex> lk(g->mu);
    LoopRound& R = g->rounds[round];
    if (++R.left == W) {  // last one out: the events have all been waited on by every stream
      for (auto e : R.ready) (void)hipEventDestroy(e);
      for (auto e : R.copied) (void)hipEventDestroy(e);
      g->rounds.erase(round);
    }
  }
  return MLAMG_OK;
}

__global__ void k_pack(const double* __restrict__ x, const int32_t* __restrict__ idx, int64_t n,
                       double* __restrict__ out) {
  int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i < n) out[i] = x[idx[i]];
}

int halo_pack(mlamg_halo* h, const double* x_ext, hipStream_t s) {
  if (h->n_send) {
    hipLaunchKernelGGL(k_pack, dim3((h->n_send + 255) / 256), dim3(256), 0, s, x_ext, h->send_idx,
                       h->n_send, h->send_buf);
    MLAMG_HIP(hipGetLastError());
  }
  return MLAMG_OK;
}

// the grouped send/recv of a packed halo, on stream s
int halo_post(mlamg_halo* h, double* x_ext, hipStream_t s) {
  if (h->nbr.empty()) return MLAMG_OK;
  MLAMG_TRY(xgroup_begin(h->c));
  for (size_t q = 0; q < h->nbr.size(); ++q) {
    if (h->send_cnt[q])
      MLAMG_TRY(xsend(h->c, h->send_buf + h->send_off[q], (size_t)h->send_cnt[q], h->nbr[q], s));
    if (h->recv_cnt[q])
      MLAMG_TRY(xrecv(h->c, x_ext + h->n_own + h->recv_off[q], (size_t)h->recv_cnt[q],
                      h->nbr[q], s));
  }
  return xgroup_end(h->c, s);
}

int halo_exchange_impl(mlamg_halo* h, double* x_ext, hipStream_t s) {
  MLAMG_TRY(halo_pack(h, x_ext, s));
  return halo_post(h, x_ext, s);
}

// what the executor reads of a communicator and of a halo (comm.hpp)
int comm_rank(const mlamg_comm* c) { return c->rank; }
int comm_size(const mlamg_comm* c) { return c->nranks; }
bool comm_is_loopback(const mlamg_comm* c) { return c->loop != nullptr; }
int64_t halo_owned(const mlamg_halo* h) { return h->n_own; }
int64_t halo_ghosts(const mlamg_halo* h) { return h->n_ghost; }
bool halo_has_neighbours(const mlamg_halo* h) { return !h->nbr.empty(); }

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_comm_unique_id(void* id_out) {
  MLAMG_REQUIRE(id_out, "NULL argument");
  ncclUniqueId id;
  MLAMG_NCCL(ncclGetUniqueId(&id));
  std::memcpy(id_out, &id, sizeof(id));
  return MLAMG_OK;
}

int mlamg_comm_create(const void* id, int nranks, int rank, mlamg_comm** out) {
  MLAMG_REQUIRE(id && out && nranks >= 1 && rank >= 0 && rank < nranks, "invalid argument");
  auto* c = new mlamg_comm();
  c->nranks = nranks;
  c->rank = rank;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  ncclResult_t r = ncclCommInitRank(&c->comm, nranks, uid, rank);
  if (r != ncclSuccess) {
    delete c;
    set_error(std::string("ncclCommInitRank failed: ") + ncclGetErrorString(r));
    return MLAMG_ENCCL;
  }
  *out = c;
  return MLAMG_OK;
}

int mlamg_comm_info(const mlamg_comm* c, int* nranks_out, int* rank_out, int* device_out,
                    int* transport_out) {
  MLAMG_REQUIRE(c && nranks_out && rank_out, "NULL argument");
  if (c->comm) {  // as RCCL itself reports them
    MLAMG_NCCL(ncclCommCount(c->comm, nranks_out));
    MLAMG_NCCL(ncclCommUserRank(c->comm, rank_out));
    if (device_out) MLAMG_NCCL(ncclCommCuDevice(c->comm, device_out));
  } else {
    *nranks_out = c->nranks;
    *rank_out = c->rank;
    if (device_out) MLAMG_HIP(hipGetDevice(device_out));
  }
  if (transport_out) *transport_out = c->comm ? 0 : (c->loop ? 1 : 2);
  return MLAMG_OK;
}

int mlamg_comm_destroy(mlamg_comm* c) {
  if (c) {
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->ar_stage) (void)hipFree(c->ar_stage);
    if (c->loop) {
      std::lock_guard<std::mutex> lk(c->loop->mu);
      --c->loop->members;
    }
    delete c;
  }
  return MLAMG_OK;
}

int mlamg_loop_group_create(int nranks, mlamg_loop_group** out) {
  MLAMG_REQUIRE(out && nranks >= 1, "invalid argument");
  auto* g = new mlamg_loop_group();
  g->W = nranks;
  g->send_seq.assign((size_t)nranks * nranks, 0);
  g->recv_seq.assign((size_t)nranks * nranks, 0);
  *out = g;
  return MLAMG_OK;
}

int mlamg_loop_group_destroy(mlamg_loop_group* g) {
  if (g) {
    {
      std::lock_guard<std::mutex> lk(g->mu);
      MLAMG_REQUIRE(g->members == 0, "loop group still has communicators");
    }
    delete g;
  }
  return MLAMG_OK;
}

int mlamg_comm_create_null(int nranks, int rank, mlamg_comm** out) {
  MLAMG_REQUIRE(out && nranks >= 1 && rank >= 0 && rank < nranks, "invalid argument");
  auto* c = new mlamg_comm();
  c->nranks = nranks;
  c->rank = rank;
  c->null_transport = true;
  *out = c;
  return MLAMG_OK;
}

int mlamg_comm_create_loopback(mlamg_loop_group* g, int rank, mlamg_comm** out) {
  MLAMG_REQUIRE(g && out && rank >= 0 && rank < g->W, "invalid argument");
  auto* c = new mlamg_comm();
  c->nranks = g->W;
  c->rank = rank;
  c->loop = g;
  {
    std::lock_guard<std::mutex> lk(g->mu);
    ++g->members;
  }
  *out = c;
  return MLAMG_OK;
}

int mlamg_comm_allreduce_sum(mlamg_comm* c, double* buf, int64_t n, void* stream) {
  MLAMG_REQUIRE(c && (n == 0 || buf), "NULL argument");
  return xallreduce_sum(c, buf, (size_t)n, S(stream));
}

int mlamg_halo_create(mlamg_comm* c, int64_t n_own, int32_t n_nbr, const int32_t* nbr,
                      const int64_t* send_cnt, const int32_t* send_idx_host,
                      const int64_t* recv_cnt, mlamg_halo** out) {
  MLAMG_REQUIRE(c && out && n_own >= 0 && n_nbr >= 0, "invalid argument");
  MLAMG_REQUIRE(n_nbr == 0 || (nbr && send_cnt && recv_cnt), "NULL argument");
  auto* h = new mlamg_halo();
  h->c = c;
  h->n_own = n_own;
  int64_t so = 0, ro = 0;
  for (int q = 0; q < n_nbr; ++q) {
    if (nbr[q] < 0 || nbr[q] >= c->nranks || nbr[q] == c->rank || send_cnt[q] < 0 || recv_cnt[q] < 0) {
      delete h;
      set_error("mlamg_halo_create: invalid neighbour entry");
      return MLAMG_EINVAL;
    }
    h->nbr.push_back(nbr[q]);
    h->send_off.push_back(so);
    h->send_cnt.push_back(send_cnt[q]);
    h->recv_off.push_back(ro);
    h->recv_cnt.push_back(recv_cnt[q]);
    so += send_cnt[q];
    ro += recv_cnt[q];
  }
  h->n_send = so;
  h->n_ghost = ro;
  for (int64_t i = 0; i < so; ++i)
    if (send_idx_host[i] < 0 || send_idx_host[i] >= n_own) {
      delete h;
      set_error("mlamg_halo_create: send index out of range");
      return MLAMG_EINVAL;
    }
  if (so) {
    if (hipMalloc(&h->send_idx, sizeof(int32_t) * so) != hipSuccess ||
        hipMalloc(&h->send_buf, sizeof(double) * so) != hipSuccess ||
        hipMemcpy(h->send_idx, send_idx_host, sizeof(int32_t) * so, hipMemcpyHostToDevice) !=
            hipSuccess) {
      if (h->send_idx) (void)hipFree(h->send_idx);
      if (h->send_buf) (void)hipFree(h->send_buf);
      delete h;
      set_error("mlamg_halo_create: device allocation failed");
      return MLAMG_ENOMEM;
    }
  }
  *out = h;
  return MLAMG_OK;
}

int mlamg_halo_destroy(mlamg_halo* h) {
  if (h) {
    if (h->send_idx) (void)hipFree(h->send_idx);
    if (h->send_buf) (void)hipFree(h->send_buf);
    delete h;
  }
  return MLAMG_OK;
}

int mlamg_halo_exchange(mlamg_halo* h, double* x_ext, void* stream) {
  MLAMG_REQUIRE(h && (h->n_own + h->n_ghost == 0 || x_ext), "NULL argument");
  return halo_exchange_impl(h, x_ext, S(stream));
}

}  // extern "C"
