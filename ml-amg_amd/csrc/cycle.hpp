// What the V-cycle executors (hier.hip, dhier.hip) share on the host side: the cache of one
// captured cycle and the batched launch loop with its pinned copy of the stop flag. (The block
// executor hier_mv.hip launches eagerly; it gets this header with the handle, hier.hpp.)
#pragma once
#include "common.hpp"

namespace mlamg {

// What a captured cycle bakes in: the caller's pointers, the tolerance and the storage formats
// (format_epoch: kernel choice and format arrays). A zero-guess coarse cycle has only b.
struct CycleKey {
  const double* b = nullptr;
  double* x = nullptr;
  double* hist = nullptr;
  double tol = kNoTol;
  uint64_t epoch = 0;
  bool operator==(const CycleKey& o) const {
    return b == o.b && x == o.x && hist == o.hist && tol == o.tol && epoch == o.epoch;
  }
};

// One captured cycle: the graph, its executable, the key it was recorded for and the stream it
// is recorded on. Empty until capture() succeeds; released with its owner.
class CycleGraph {
 public:
  CycleGraph() = default;
  CycleGraph(const CycleGraph&) = delete;
  CycleGraph& operator=(const CycleGraph&) = delete;
  ~CycleGraph() {
    invalidate();
    if (stream_) (void)hipStreamDestroy(stream_);
  }

  double* res = nullptr;  // coarse-cycle use: the buffer the recorded cycle leaves its result in

  bool current(const CycleKey& k) const { return exec_ && key_ == k; }

  void invalidate() {
    if (exec_) (void)hipGraphExecDestroy(exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    exec_ = nullptr;
    graph_ = nullptr;
  }

  // the capture stream, created on first use (a caller that must order it after earlier work
  // does so before capture())
  int stream(hipStream_t* out) {
    if (!stream_) MLAMG_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    *out = stream_;
    return MLAMG_OK;
  }

  // Replace the cached cycle by what record(capture stream) launches. Thread-local capture: the
  // loopback tests run one host thread per rank, and another rank's API calls must not break
  // this one's recording. A failed recording still ends the capture and leaves the object empty.
  template <class F>
  int capture(const CycleKey& k, F&& record) {
    invalidate();
    hipStream_t cs = nullptr;
    MLAMG_TRY(stream(&cs));
    MLAMG_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = record(cs);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc != MLAMG_OK) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    MLAMG_HIP(e);
    graph_ = g;
    const hipError_t ei = hipGraphInstantiate(&exec_, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) invalidate();
    MLAMG_HIP(ei);
    key_ = k;
    return MLAMG_OK;
  }

  int launch(hipStream_t s) const {
    MLAMG_HIP(hipGraphLaunch(exec_, s));
    return MLAMG_OK;
  }

 private:
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
  CycleKey key_;
  hipStream_t stream_ = nullptr;
};

// Pinned host copy of a device stop flag, allocated on first use and freed with its owner.
// get() may return nullptr (allocation failed): run_cycles then launches every cycle.
struct DoneHost {
  int32_t* p = nullptr;
  DoneHost() = default;
  DoneHost(const DoneHost&) = delete;
  DoneHost& operator=(const DoneHost&) = delete;
  ~DoneHost() {
    if (p) (void)hipHostFree(p);
  }
  int32_t* get() {
    if (!p) (void)hipHostMalloc(&p, sizeof(int32_t), hipHostMallocDefault);
    return p;
  }
};

// Cycles are launched in batches; with a tolerance, the device-side stop flag is read back
// after each batch so the cycles after convergence are not launched at all (each would only
// check the flag and return, ~10 launches apiece). Batches grow 4, 4, 8, 16, 32, 32, ...: at
// most one batch of overshoot, a host sync per batch.
template <class F>
static int run_cycles(int n_cycles, double tol, int32_t* done_dev, DoneHost& done, hipStream_t s,
                      F&& one) {
  int32_t* done_host = done.get();
  if (!(tol >= 0.0) || !done_host) {
    for (int c = 0; c < n_cycles; ++c) MLAMG_TRY(one());
    return MLAMG_OK;
  }
  int c = 0, batch = 4, k = 0;
  while (c < n_cycles) {
    const int m = std::min(batch, n_cycles - c);
    for (int i = 0; i < m; ++i) MLAMG_TRY(one());
    c += m;
    if (c >= n_cycles) break;
    MLAMG_HIP(hipMemcpyAsync(done_host, done_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MLAMG_HIP(hipStreamSynchronize(s));
    if (*done_host) break;
    if (++k >= 2) batch = std::min(batch * 2, 32);
  }
  return MLAMG_OK;
}

}  // namespace mlamg
