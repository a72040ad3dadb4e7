// Multi-GPU V-cycle: the partitioned V(1,1) executor, over the transport of comm.hip.
//
// One process per GPU. The first K levels are row-partitioned (mlamg/partition.py builds the
// maps: level 0 in near-equal blocks, level l+1 owned by the rank owning each aggregate's
// seed); the levels below are replicated on every rank (their setup is deterministic) and run
// as the zero-guess cycle of an ordinary mlamg_hier. Vectors are x_ext = [owned | ghosts]. One
// cycle of partitioned level l, whose first pre-smoothing sweep has already been applied (l = 0:
// x += Dinv r by the caller before the first cycle and by the end of the previous cycle after
// that; l > 0: x = Dinv b, the zero-guess sweep, by the restriction kernel of the level above):
//   halo_x(x); r = b - A_loc x_ext
//   halo_r(r); b_{l+1}[own] = R_own r_ext             coarse rows summed by their owner
//   l+1 partitioned:  (same kernel) x_{l+1} = Dinv b_{l+1}; cycle below; halo_p(x_{l+1})
//   else (replicated tail):  allgatherv(b_{l+1}); x_{l+1} = replicated cycle, on every rank
//   x += P_loc x_{l+1,ext}           owned AND ghost rows: no halo before the post-smoothing
//   t = x + Dinv (b - A_loc x_ext)                    post-smoothing
//   l = 0: halo_x(t); r = b - A t with per-block partials of ||r||^2, and in the same kernel
//          x = t + Dinv r (the next cycle's first sweep); rank sum, all-reduce, sqrt -> history
//          and stop flag (MLAMG.py:194). After the last cycle the caller copies t back into x.
// Overlap split (exchange_then): an operator behind a halo may come split into rows that read
// no ghost and the rows before and after them; the exchange then runs on a second stream while
// the interior rows run, and the boundary rows follow the join.
// Local rows keep their stored order and every coarse row is summed by one owner, so the
// iterate is bitwise the single-GPU iterate; only the norm's summation order differs.
// A whole cycle (kernels and RCCL calls) can be replayed from one captured graph (cycle.hpp);
// otherwise the replicated tail alone replays its own.
#include "comm.hpp"
#include "cycle.hpp"
#include "reduce.hpp"

namespace mlamg {

// sum the residual partials of this rank into partial[n] (fixed order)
__global__ __launch_bounds__(1024) void k_local_sum(double* __restrict__ partial, int n) {
  __shared__ double red[16];
  const double t = partials_total<1024>(partial, n, red);
  if (threadIdx.x == 0) partial[n] = t;
}

__global__ void k_norm_finish(const double* __restrict__ sum, double* hist, int32_t* counter,
                              int32_t* done, double tol) {
  if (*done) return;  // converged earlier: every rank saw the same global norm
  const double nrm = sqrt(*sum);
  const int c = *counter;
  if (hist) hist[c] = nrm;
  *counter = c + 1;
  if (tol >= 0.0 && nrm <= tol) *done = 1;
}

}  // namespace mlamg

using namespace mlamg;

namespace {
// An operator split by rows for overlapping its halo exchange: part 1 is a run
// of rows that read no ghost entry, parts 0 and 2 the rows before and after it (either may be
// empty). Part k holds rows [r0[k], r0[k] + rows) of the operator, stored in the same order and
// in an exact-order kernel format, so every row's sum is the unsplit operator's bit for bit.
struct OpSplit {
  const mlamg_csr* m[3] = {nullptr, nullptr, nullptr};
  int64_t r0[3] = {0, 0, 0};
  bool on() const { return m[1] != nullptr; }
};

struct DLevel {
  const mlamg_csr* A = nullptr;  // n_own x (n_own + ghosts_x)
  const mlamg_csr* P = nullptr;  // n_own x (next own + ghosts_p) | n_own x n_c (last level)
  const mlamg_csr* R = nullptr;  // next own x (n_own + ghosts_r)
  const double* dinv = nullptr;
  mlamg_halo* hx = nullptr;
  mlamg_halo* hr = nullptr;
  mlamg_halo* hp = nullptr;  // halo of x_{l+1} for P (nullptr on the last partitioned level)
  OpSplit sA, sR, sP;        // row splits behind hx, hr, hp (optional)
  int64_t n_own = 0;
  // work (l > 0: x_ext, b own; every level: r_ext, t_ext; xp_ext = x_{l+1} for P)
  double* x_ext = nullptr;
  double* b = nullptr;
  double* r_ext = nullptr;
  double* t_ext = nullptr;
  double* xp_ext = nullptr;
};
}  // namespace

struct mlamg_dhier {
  mlamg_comm* c = nullptr;
  int rank = 0, world = 1;  // of c
  std::vector<DLevel> lv;
  mlamg_hier* coarse = nullptr;  // replicated levels K..L
  std::vector<int64_t> c_lo_all, c_hi_all;  // owned segments of the replicated space
  int64_t nc = 0;
  double* bc = nullptr;
  double* partial = nullptr;
  int32_t* flags = nullptr;  // counter, done
  std::vector<void*> bufs;
  bool ready = false;
  int coarse_graph = 1;
  // whole-cycle hipGraph (kernels + RCCL calls captured together), keyed like mlamg_hier's
  int cycle_graph = 0;
  bool capturing = false;
  CycleGraph graph;
  DoneHost done_host;  // pinned copy of the stop flag (run_cycles)
  // halo / interior overlap: the RCCL group of a split operator's exchange runs on comm_s while
  // the interior rows run on the cycle's stream (events fork and join the two)
  int overlap = 1;
  hipStream_t comm_s = nullptr;
  std::vector<hipEvent_t> evs;
  size_t ev_next = 0;
};

// the exchange of halo h into buf followed by the operator `whole`, through op(M, row0, part):
// unsplit, the exchange then op(whole, 0, -1); split, the pack on s, the RCCL group on comm_s
// (forked from s after the pack, so every earlier reader of the ghost region is done), the
// interior rows on s meanwhile, then s joins comm_s and runs the boundary rows
template <class Op>
static int exchange_then(mlamg_dhier* D, mlamg_halo* h, double* buf, const mlamg_csr* whole,
                         const OpSplit& sp, hipStream_t s, Op&& op) {
  if (!(D->overlap && sp.on() && halo_has_neighbours(h))) {
    MLAMG_TRY(halo_exchange_impl(h, buf, s));
    return op(whole, (int64_t)0, -1);
  }
  if (D->ev_next + 2 > D->evs.size()) {
    for (int q = 0; q < 16; ++q) {
      hipEvent_t e;
      MLAMG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      D->evs.push_back(e);
    }
  }
  hipEvent_t fork = D->evs[D->ev_next++], join = D->evs[D->ev_next++];
  MLAMG_TRY(halo_pack(h, buf, s));
  MLAMG_HIP(hipEventRecord(fork, s));
  MLAMG_HIP(hipStreamWaitEvent(D->comm_s, fork, 0));
  MLAMG_TRY(halo_post(h, buf, D->comm_s));
  MLAMG_HIP(hipEventRecord(join, D->comm_s));
  MLAMG_TRY(op(sp.m[1], sp.r0[1], 1));
  MLAMG_HIP(hipStreamWaitEvent(s, join, 0));
  if (sp.m[0]) MLAMG_TRY(op(sp.m[0], sp.r0[0], 0));
  if (sp.m[2]) MLAMG_TRY(op(sp.m[2], sp.r0[2], 2));
  return MLAMG_OK;
}

static int dalloc(mlamg_dhier* D, double** p, int64_t n) {
  void* q = nullptr;
  MLAMG_HIP(hipMalloc(&q, sizeof(double) * std::max<int64_t>(n, 1)));
  MLAMG_HIP(hipMemset(q, 0, sizeof(double) * std::max<int64_t>(n, 1)));
  D->bufs.push_back(q);
  *p = static_cast<double*>(q);
  return MLAMG_OK;
}

static int dprepare(mlamg_dhier* D) {
  if (D->ready) return MLAMG_OK;
  MLAMG_REQUIRE(!D->lv.empty(), "no partitioned level");
  MLAMG_REQUIRE(D->lv.back().hp == nullptr, "last partitioned level must have halo_p = NULL");
  for (size_t l = 0; l < D->lv.size(); ++l) {
    DLevel& L = D->lv[l];
    const int64_t ext = L.n_own + std::max(halo_ghosts(L.hx), halo_ghosts(L.hr));
    if (l > 0) {
      MLAMG_TRY(dalloc(D, &L.x_ext, ext));
      MLAMG_TRY(dalloc(D, &L.b, L.n_own));
    }
    MLAMG_TRY(dalloc(D, &L.r_ext, ext));
    // t_ext of level l > 0 doubles as the P-halo buffer (xp_ext) of level l - 1
    const int64_t pg = l > 0 ? halo_ghosts(D->lv[l - 1].hp) : 0;
    MLAMG_TRY(dalloc(D, &L.t_ext, std::max(ext, L.n_own + pg)));
    if (l > 0) D->lv[l - 1].xp_ext = L.t_ext;
  }
  MLAMG_TRY(dalloc(D, &D->bc, D->nc));
  int64_t pc = part_capacity(D->lv[0].A), ps = 0;
  for (int k = 0; k < 3; ++k)
    if (D->lv[0].sA.m[k]) ps += part_capacity(D->lv[0].sA.m[k]);
  MLAMG_TRY(dalloc(D, &D->partial, std::max(pc, ps)));
  if (!D->comm_s) MLAMG_HIP(hipStreamCreateWithFlags(&D->comm_s, hipStreamNonBlocking));
  double* f = nullptr;
  MLAMG_TRY(dalloc(D, &f, 1));
  D->flags = reinterpret_cast<int32_t*>(f);
  // the zero fills run on the null stream and may still be in flight: finish them before work
  // on the caller's (possibly non-blocking) stream touches these buffers
  MLAMG_HIP(hipDeviceSynchronize());
  D->ready = true;
  return MLAMG_OK;
}

// allgatherv of the owned coarse segments into the replicated b_c
static int allgather_segments(mlamg_dhier* D, hipStream_t s) {
  const int P = D->world, me = D->rank;
  if (P == 1) return MLAMG_OK;
  const int64_t lo = D->c_lo_all[me];
  const size_t mine = (size_t)(D->c_hi_all[me] - lo);
  MLAMG_TRY(xgroup_begin(D->c));
  for (int q = 0; q < P; ++q) {
    if (q == me) continue;
    if (mine) MLAMG_TRY(xsend(D->c, D->bc + lo, mine, q, s));
    const size_t theirs = (size_t)(D->c_hi_all[q] - D->c_lo_all[q]);
    if (theirs) MLAMG_TRY(xrecv(D->c, D->bc + D->c_lo_all[q], theirs, q, s));
  }
  return xgroup_end(D->c, s);
}

static int dcycle_below(mlamg_dhier* D, size_t l, double** x_out, hipStream_t s);

// coarse-grid correction of partitioned level l: b_{l+1} = R r, solve below, x += P x_{l+1}
static int correct(mlamg_dhier* D, size_t l, double* x_ext, const int32_t* done, hipStream_t s) {
  DLevel& L = D->lv[l];
  if (L.hp) {
    DLevel& N = D->lv[l + 1];
    // restriction fused with the next level's zero-guess sweep (x = Dinv_w b on owned rows)
    MLAMG_TRY(exchange_then(D, L.hr, L.r_ext, L.R, L.sR, s,
                            [&](const mlamg_csr* M, int64_t r0, int) {
                              return spmv_set(M, L.r_ext, N.b + r0, done, s, N.x_ext + r0,
                                              N.dinv + r0);
                            }));
    double* xn = nullptr;
    MLAMG_TRY(dcycle_below(D, l + 1, &xn, s));
    // xp_ext is the level below's t_ext: its owned part is the correction, the P-halo lands in
    // its (no longer needed) ghost region. P rows cover the owned AND the x-ghost rows: x_ext's
    // ghosts get the same update their owners compute (same row, same order, same inputs), so
    // no x halo is needed afterwards
    MLAMG_TRY(exchange_then(D, L.hp, L.xp_ext, L.P, L.sP, s,
                            [&](const mlamg_csr* M, int64_t r0, int) {
                              return spmv_add(M, L.xp_ext, x_ext + r0, done, s);
                            }));
  } else {
    double* bo = D->bc + D->c_lo_all[D->rank];
    MLAMG_TRY(exchange_then(D, L.hr, L.r_ext, L.R, L.sR, s,
                            [&](const mlamg_csr* M, int64_t r0, int) {
                              return spmv_set(M, L.r_ext, bo + r0, done, s);
                            }));
    MLAMG_TRY(allgather_segments(D, s));
    double* xc = nullptr;
    // inside a whole-cycle capture the coarse kernels are captured directly (no nested graph)
    MLAMG_TRY(hier_coarse_cycle(D->coarse, D->bc, &xc, D->coarse_graph && !D->capturing, s));
    MLAMG_TRY(spmv_add(L.P, xc, x_ext, done, s));
  }
  return MLAMG_OK;
}

// one cycle from a zero guess at partitioned level l > 0 (rhs in lv[l].b); result (own part)
// returned through x_out
static int dcycle_below(mlamg_dhier* D, size_t l, double** x_out, hipStream_t s) {
  const int32_t* done = D->flags + 1;
  DLevel& L = D->lv[l];
  // x = Dinv_w b was written by the restriction kernel of the level above (correct())
  MLAMG_TRY(exchange_then(D, L.hx, L.x_ext, L.A, L.sA, s,
                          [&](const mlamg_csr* M, int64_t r0, int) {
                            return residual_impl(M, L.b + r0, L.x_ext, L.r_ext + r0, nullptr,
                                                 nullptr, nullptr, const_cast<int32_t*>(done),
                                                 kNoTol, nullptr, nullptr, nullptr, s);
                          }));
  MLAMG_TRY(correct(D, l, L.x_ext, done, s));
  MLAMG_TRY(jacobi_sweep(L.A, L.dinv, L.b, L.x_ext, L.t_ext, false, done, s));
  *x_out = L.t_ext;
  return MLAMG_OK;
}

// Fused as in hier.hip: the end-of-cycle residual kernel also writes x = t + Dinv_w r (the next
// cycle's first pre-smoothing sweep); the caller applies the first sweep before the first cycle
// and copies t (still in t_ext) back into x after the last.
static int dcycle(mlamg_dhier* D, const double* b, double* x_ext, double* hist, double tol,
                  hipStream_t s) {
  int32_t* counter = D->flags;
  int32_t* done = D->flags + 1;
  DLevel& L = D->lv[0];
  const mlamg_csr* A = L.A;
  D->ev_next = 0;
  MLAMG_TRY(exchange_then(D, L.hx, x_ext, A, L.sA, s, [&](const mlamg_csr* M, int64_t r0, int) {
    return residual_impl(M, b ? b + r0 : nullptr, x_ext, L.r_ext + r0, nullptr, nullptr, nullptr,
                         done, kNoTol, nullptr, nullptr, nullptr, s);
  }));
  MLAMG_TRY(correct(D, 0, x_ext, done, s));
  MLAMG_TRY(jacobi_sweep(A, L.dinv, b, x_ext, L.t_ext, false, done, s));
  // r = b - A t with per-block ||r||^2 partials, x <- t; then the global norm
  // (r itself is not stored: the next cycle starts with its own residual). Split: the parts'
  // partials lie in part order (0, 1, 2), whatever order the parts ran in. The parts' row
  // blocks are cut differently from the unsplit operator's, so the NORM (history, tolerance
  // stop) matches overlap-off / single-GPU runs to rounding, not bitwise; the iterate itself is
  // bitwise unchanged (every row is summed in its stored order)
  int64_t poff[3] = {0, 0, 0};
  int nb = (int)A->n_part;
  if (D->overlap && L.sA.on() && halo_has_neighbours(L.hx)) {
    nb = 0;
    for (int k = 0; k < 3; ++k) {
      poff[k] = nb;
      if (L.sA.m[k]) nb += (int)L.sA.m[k]->n_part;
    }
  }
  MLAMG_TRY(exchange_then(D, L.hx, L.t_ext, A, L.sA, s,
                          [&](const mlamg_csr* M, int64_t r0, int part) {
                            return residual_partials(M, b ? b + r0 : nullptr, L.t_ext, nullptr,
                                                     x_ext + r0,
                                                     L.t_ext + r0,
                                                     D->partial + (part < 0 ? 0 : poff[part]),
                                                     done, s, L.dinv + r0);
                          }));
  hipLaunchKernelGGL(k_local_sum, dim3(1), dim3(1024), 0, s, D->partial, nb);
  MLAMG_HIP(hipGetLastError());
  if (D->world > 1) MLAMG_TRY(xallreduce_sum(D->c, D->partial + nb, 1, s));
  hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(1), 0, s, D->partial + nb, hist, counter, done,
                     tol);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// Record one dcycle into D->graph. Everything a capture must not contain happens first: the
// caller has run one cycle eagerly (RCCL sets up its peer connections on first use), the
// replicated tail allocates its work buffers, and the capture stream is ordered after the work
// already queued on s and drained.
static int dcapture(mlamg_dhier* D, const CycleKey& key, hipStream_t s) {
  MLAMG_TRY(hier_prepare_ext(D->coarse));
  hipStream_t cs = nullptr;
  MLAMG_TRY(D->graph.stream(&cs));
  hipEvent_t ev;
  MLAMG_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  MLAMG_HIP(hipEventRecord(ev, s));
  MLAMG_HIP(hipStreamWaitEvent(cs, ev, 0));
  MLAMG_HIP(hipStreamSynchronize(cs));
  (void)hipEventDestroy(ev);
  return D->graph.capture(key, [&](hipStream_t cap) {
    D->capturing = true;
    const int rc = dcycle(D, key.b, key.x, key.hist, key.tol, cap);
    D->capturing = false;
    return rc;
  });
}

extern "C" {

int mlamg_dhier_create(mlamg_comm* c, mlamg_hier* coarse, int64_t nc, const int64_t* c_lo_all,
                       const int64_t* c_hi_all, mlamg_dhier** out) {
  MLAMG_REQUIRE(c && coarse && c_lo_all && c_hi_all && out, "NULL argument");
  auto* D = new mlamg_dhier();
  D->c = c;
  D->rank = comm_rank(c);
  D->world = comm_size(c);
  D->coarse = coarse;
  D->nc = nc;
  D->c_lo_all.assign(c_lo_all, c_lo_all + D->world);
  D->c_hi_all.assign(c_hi_all, c_hi_all + D->world);
  for (int q = 0; q < D->world; ++q)
    if (D->c_lo_all[q] < 0 || D->c_hi_all[q] < D->c_lo_all[q] || D->c_hi_all[q] > nc ||
        (q > 0 && D->c_lo_all[q] != D->c_hi_all[q - 1])) {
      delete D;
      set_error("mlamg_dhier_create: coarse segments must tile [0, nc) in rank order");
      return MLAMG_EINVAL;
    }
  *out = D;
  return MLAMG_OK;
}

int mlamg_dhier_add_level(mlamg_dhier* D, const mlamg_csr* A_loc, const double* dinv_w,
                          const mlamg_csr* P_loc, const mlamg_csr* R_own, mlamg_halo* halo_x,
                          mlamg_halo* halo_r, mlamg_halo* halo_p) {
  MLAMG_REQUIRE(D && A_loc && dinv_w && P_loc && R_own && halo_x && halo_r, "NULL argument");
  MLAMG_REQUIRE(!D->ready, "hierarchy already in use");
  const int64_t n = A_loc->n_rows;
  MLAMG_REQUIRE(A_loc->n_cols == n + halo_ghosts(halo_x), "A_loc columns != n_own + x ghosts");
  MLAMG_REQUIRE(halo_owned(halo_x) == n && halo_owned(halo_r) == n, "halo n_own mismatch");
  MLAMG_REQUIRE(P_loc->n_rows == n + halo_ghosts(halo_x), "P_loc rows != n_own + x ghosts");
  MLAMG_REQUIRE(R_own->n_cols == n + halo_ghosts(halo_r), "R_own columns != n_own + r ghosts");
  if (!D->lv.empty()) {
    DLevel& up = D->lv.back();
    MLAMG_REQUIRE(up.hp != nullptr, "previous level was declared the last partitioned level");
    MLAMG_REQUIRE(up.R->n_rows == n, "level rows != owned coarse rows of the level above");
    MLAMG_REQUIRE(halo_owned(up.hp) == n, "P halo of the level above has a different n_own");
    MLAMG_REQUIRE(up.P->n_cols == n + halo_ghosts(up.hp), "P_loc columns != next own + p ghosts");
  }
  if (!halo_p) {
    const int me = D->rank;
    MLAMG_REQUIRE(P_loc->n_cols == D->nc, "last level P must have the replicated coarse columns");
    MLAMG_REQUIRE(R_own->n_rows == D->c_hi_all[me] - D->c_lo_all[me],
                  "R_own rows != owned coarse segment");
  }
  DLevel L;
  L.A = A_loc;
  L.P = P_loc;
  L.R = R_own;
  L.dinv = dinv_w;
  L.hx = halo_x;
  L.hr = halo_r;
  L.hp = halo_p;
  L.n_own = n;
  D->lv.push_back(L);
  return MLAMG_OK;
}

int mlamg_dhier_set_split(mlamg_dhier* D, int level, int which, const mlamg_csr* lo,
                          const mlamg_csr* mid, const mlamg_csr* hi) {
  MLAMG_REQUIRE(D && mid, "NULL argument");
  MLAMG_REQUIRE(!D->ready, "hierarchy already in use");
  MLAMG_REQUIRE(level >= 0 && (size_t)level < D->lv.size(), "level out of range");
  MLAMG_REQUIRE(which >= 0 && which <= 2, "which: 0 = A, 1 = R, 2 = P");
  DLevel& L = D->lv[level];
  MLAMG_REQUIRE(which != 2 || L.hp, "P is split only where a P halo precedes it");
  const mlamg_csr* whole = which == 0 ? L.A : which == 1 ? L.R : L.P;
  OpSplit sp;
  sp.m[0] = lo;
  sp.m[1] = mid;
  sp.m[2] = hi;
  int64_t r = 0;
  for (int k = 0; k < 3; ++k) {
    sp.r0[k] = r;
    if (!sp.m[k]) continue;
    MLAMG_REQUIRE(sp.m[k]->n_cols == whole->n_cols, "split part has other columns");
    // the row-pair kernels load epilogue vectors as 16-byte pairs: parts start on even rows
    MLAMG_REQUIRE(r % 2 == 0, "split parts must start on even rows");
    r += sp.m[k]->n_rows;
  }
  MLAMG_REQUIRE(r == whole->n_rows, "split parts do not cover the operator's rows");
  (which == 0 ? L.sA : which == 1 ? L.sR : L.sP) = sp;
  return MLAMG_OK;
}

int mlamg_dhier_set_overlap(mlamg_dhier* D, int on) {
  MLAMG_REQUIRE(D, "NULL argument");
  D->overlap = on ? 1 : 0;
  D->graph.invalidate();
  return MLAMG_OK;
}

int mlamg_dhier_destroy(mlamg_dhier* D) {
  if (D) {
    if (D->comm_s) (void)hipStreamDestroy(D->comm_s);
    for (hipEvent_t e : D->evs) (void)hipEventDestroy(e);
    for (void* p : D->bufs)
      if (p) (void)hipFree(p);
    delete D;
  }
  return MLAMG_OK;
}

int mlamg_dhier_set_coarse_graph(mlamg_dhier* D, int use_graph) {
  MLAMG_REQUIRE(D, "NULL argument");
  D->coarse_graph = use_graph;
  return MLAMG_OK;
}

int mlamg_dhier_set_cycle_graph(mlamg_dhier* D, int use_graph) {
  MLAMG_REQUIRE(D, "NULL argument");
  D->cycle_graph = use_graph;
  D->graph.invalidate();
  return MLAMG_OK;
}

int mlamg_dhier_vcycle(mlamg_dhier* D, const double* b, double* x_ext, int n_cycles, double tol,
                       double* res_hist, int32_t* cycles_done_host, void* stream) {
  // b NULL: this rank's part of the right-hand side is zero (as mlamg_hier_vcycle: the
  // fine-level kernels take +0.0 instead of reading b; same bits)
  MLAMG_REQUIRE(D && x_ext, "NULL argument");
  MLAMG_REQUIRE(n_cycles >= 0, "n_cycles < 0");
  MLAMG_TRY(dprepare(D));
  hipStream_t s = S(stream);
  DLevel& L = D->lv[0];
  MLAMG_HIP(hipMemsetAsync(D->flags, 0, 2 * sizeof(int32_t), s));
  MLAMG_TRY(halo_exchange_impl(L.hx, x_ext, s));
  MLAMG_TRY(residual_impl(L.A, b, x_ext, L.r_ext, nullptr, nullptr, nullptr, nullptr, kNoTol,
                          nullptr, nullptr, nullptr, s));
  if (n_cycles > 0) {
    // the first cycle's first pre-smoothing sweep (later ones are fused into the cycle end)
    MLAMG_TRY(jacobi_from_residual(x_ext, L.dinv, L.r_ext, L.n_own, nullptr, s));
    MLAMG_REQUIRE(!(D->cycle_graph && comm_is_loopback(D->c)),
                  "the loopback transport cannot be captured into a graph");
    int c0 = 0;
    const CycleKey key{b, x_ext, res_hist, tol, format_epoch()};
    if (D->cycle_graph && !D->graph.current(key)) {
      // the first cycle runs eagerly: every RCCL peer connection (halo neighbours, the
      // allgather of coarse segments, the norm all-reduce) is set up outside the capture
      MLAMG_TRY(dcycle(D, b, x_ext, res_hist, tol, s));
      c0 = 1;
      MLAMG_TRY(dcapture(D, key, s));
    }
    // every rank reads the same flag (set from the all-reduced norm) after the same batch,
    // so all ranks launch the same number of cycles and their collectives stay matched
    MLAMG_TRY(run_cycles(n_cycles - c0, tol, D->flags + 1, D->done_host, s, [&]() {
      return D->cycle_graph ? D->graph.launch(s) : dcycle(D, b, x_ext, res_hist, tol, s);
    }));
    // the iterate is t; x holds t + Dinv_w r for a cycle that never ran
    MLAMG_HIP(hipMemcpyAsync(x_ext, L.t_ext, sizeof(double) * L.n_own, hipMemcpyDeviceToDevice, s));
  }
  if (cycles_done_host) {
    int32_t cnt = 0;
    MLAMG_HIP(hipMemcpyAsync(&cnt, D->flags, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MLAMG_HIP(hipStreamSynchronize(s));
    *cycles_done_host = cnt;
  }
  return MLAMG_OK;
}

}  // extern "C"
