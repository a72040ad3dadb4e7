// Gauss-Seidel sweeps on a block of k vectors (row-major n x k multivectors, include/mlamg.h):
// the level schedule of gs.hip walked once for all k columns. A sweep's cost per dependency level
// is its chain (gather x, ordered sum, divide, store, barrier), not its bytes, so the k columns
// share it: every step of the chain does k independent ordered sums.
//
// A work item is (position in the level, column pair); pairs run fastest across lanes, so the
// ceil(k/2) lanes of a row read one contiguous run of X[col, :] per entry, each lane holding two
// accumulators, and the row's (col, val) loads are one address per row. Every column of a row is
// summed in stored order with gs_init / gs_acc / gs_fin / gs_upd, the last stored diagonal entry
// counts, and B is read straight from B[row, :]: COLUMN j OF THE RESULT IS BITWISE
// mlamg_gs_sweep ON COLUMN j.
#include "gs.hpp"

#include <cstdlib>

namespace mlamg {

// The walk takes a schedule whose widest level has at most this many items (rows x column
// pairs): 4 passes of the workgroup per level on the packed copy, 2 on the CSR arrays (whose
// passes chase rows[] -> indptr -> entries -> x); wider ones go one launch per level. Measured
// (DESIGN.md §21): a packed pass costs 0.7-1.1 us a level against 3.6-4.7 us for a launch per
// level, which the walk exceeds between 4 and 8 passes on both 2-D grids; the CSR walk of
// poisson_3d_7pt(64) (3 passes) took 5x the per-level launches.
constexpr int64_t kGsMvWalkItems = 4 * kGsBlock;
constexpr int64_t kGsMvWalkItemsCsr = 2 * kGsBlock;

// a lane's column pair at p: one 16-byte access (VEC: p is 16-byte aligned and k is even, so
// every lane has two columns) or two 8-byte ones. The lane of an odd k's last column reads that
// column twice and stores it once: no load sits behind a branch (a branch join makes the compiler
// wait for every load in flight, gs.hip k_gs_ring; measured here as +0.6 us a level).
template <bool VEC>
__device__ __forceinline__ void mv_ld2(const double* p, bool two, double& a, double& b) {
  if (VEC) {
    const double2 v = *reinterpret_cast<const double2*>(p);
    a = v.x;
    b = v.y;
  } else {
    a = p[0];
    b = p[two ? 1 : 0];
  }
}
template <bool VEC>
__device__ __forceinline__ void mv_st2(double* p, bool two, double a, double b) {
  if (VEC) {
    *reinterpret_cast<double2*>(p) = make_double2(a, b);
  } else {
    p[0] = a;
    if (two) p[1] = b;
  }
}
// the lane's b: B is the caller's block, or, for a zero right-hand side, any readable block of
// the same shape (the iterate) whose values are selected away
template <bool VEC>
__device__ __forceinline__ void mv_ldb(const double* p, bool two, bool has_b, double& a,
                                       double& b) {
  mv_ld2<VEC>(p, two, a, b);
  a = has_b ? a : 0.0;
  b = has_b ? b : 0.0;
}

// row i of the CSR arrays on columns c0, c0 + 1 (gs_row on each): four entries' loads in flight,
// then their ordered steps. The gather of the diagonal entry's own row is issued and not used.
template <bool BLK, bool VEC>
__device__ __forceinline__ void gs_mv_row(const int32_t* __restrict__ ip,
                                          const int32_t* __restrict__ ij,
                                          const double* __restrict__ ax, int32_t i, int c0,
                                          bool two, double* X, int64_t ldx, const double* B,
                                          int64_t ldb, bool has_b) {
  double b0, b1;
  mv_ldb<VEC>(B + (int64_t)i * ldb + c0, two, has_b, b0, b1);
  double s0 = gs_init<BLK>(b0), s1 = gs_init<BLK>(b1), diag = 0.0;
  const double* xc = X + c0;
  int32_t e = ip[i];
  const int32_t z = ip[i + 1];
  for (; e + 4 <= z; e += 4) {
    int32_t c[4];
    double a[4], x0[4], x1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      c[u] = ij[e + u];
      a[u] = ax[e + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) mv_ld2<VEC>(xc + (int64_t)c[u] * ldx, two, x0[u], x1[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (c[u] == i) {
        diag = a[u];
      } else {
        s0 = gs_acc<BLK>(s0, a[u], x0[u]);
        s1 = gs_acc<BLK>(s1, a[u], x1[u]);
      }
    }
  }
  for (; e < z; ++e) {
    const int32_t j = ij[e];
    const double a = ax[e];
    double x0, x1;
    mv_ld2<VEC>(xc + (int64_t)j * ldx, two, x0, x1);
    if (j == i) {
      diag = a;
    } else {
      s0 = gs_acc<BLK>(s0, a, x0);
      s1 = gs_acc<BLK>(s1, a, x1);
    }
  }
  if (BLK) diag = diag != 0.0 ? 1.0 / diag : 0.0;
  if (gs_upd<BLK>(diag))
    mv_st2<VEC>(X + (int64_t)i * ldx + c0, two, gs_fin<BLK>(s0, b0, diag),
                gs_fin<BLK>(s1, b1, diag));
}

// One level over the whole chip: item t = blockIdx.x * 256 + threadIdx.x is (position t / KP,
// pair t % KP) of the level's cnt rows, KP = ceil(k / 2). For wide levels.
template <bool BLK, bool VEC>
__global__ __launch_bounds__(256) void k_gs_mv_level(const int32_t* __restrict__ ip,
                                                     const int32_t* __restrict__ ij,
                                                     const double* __restrict__ ax,
                                                     const int32_t* __restrict__ rows,
                                                     int32_t cnt, double* X, int64_t ldx,
                                                     const double* B, int64_t ldb,
                                                     bool has_b, int k, const int32_t* done) {
  if (done && *done) return;
  const int kp = (k + 1) >> 1;
  const int64_t t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= (int64_t)cnt * kp) return;
  const int32_t pos = (int32_t)(t / kp);
  const int c0 = 2 * (int)(t - (int64_t)pos * kp);
  gs_mv_row<BLK, VEC>(ip, ij, ax, rows[pos], c0, c0 + 1 < k, X, ldx, B, ldb, has_b);
}

// a position's packed structure (gs.hpp: PK off-diagonal slots, column -1 pads) and its row id
template <int PK>
struct GsMvRow {
  int32_t row;
  int32_t col[PK];
  double val[PK];
};

// independent loads only: slots as 16-byte accesses (PK is 4 or 8, the copies are 256-byte
// aligned allocations)
template <int PK>
__device__ __forceinline__ void gs_mv_struct(GsMvRow<PK>& q, int64_t p,
                                             const int32_t* __restrict__ rows,
                                             const int32_t* __restrict__ pcol,
                                             const double* __restrict__ pval) {
  q.row = rows[p];
#pragma unroll
  for (int u = 0; u < PK; u += 4) {
    const int4 c = *reinterpret_cast<const int4*>(pcol + p * PK + u);
    q.col[u] = c.x;
    q.col[u + 1] = c.y;
    q.col[u + 2] = c.z;
    q.col[u + 3] = c.w;
  }
#pragma unroll
  for (int u = 0; u < PK; u += 2) {
    const double2 v = *reinterpret_cast<const double2*>(pval + p * PK + u);
    q.val[u] = v.x;
    q.val[u + 1] = v.y;
  }
}

// One packed row on columns c0, c0 + 1: the gathers first (they alone depend on the level
// before; a pad's gather reads row 0 and is selected away), then the row's diagonal and b, which
// come back with them, then the ordered steps. The columns are folded into a bit mask once the
// gathers are out, so their registers are free for the next level's structure.
template <bool BLK, bool VEC, int PK, class Between>
__device__ __forceinline__ void gs_mv_packed_row(const GsMvRow<PK>& q, int64_t p, bool live,
                                                 int c0, bool two,
                                                 const double* __restrict__ pdiag, double* X,
                                                 int64_t ldx, const double* B, int64_t ldb,
                                                 bool has_b, Between&& between) {
  double x0[PK], x1[PK];
  uint32_t used = 0;
#pragma unroll
  for (int u = 0; u < PK; ++u) {
    const int32_t c = q.col[u] >= 0 ? q.col[u] : 0;
    used |= (uint32_t)(q.col[u] >= 0) << u;
    mv_ld2<VEC>(X + (int64_t)c * ldx + c0, two, x0[u], x1[u]);
  }
  const double diag = pdiag[p];
  double b0, b1;
  mv_ldb<VEC>(B + (int64_t)q.row * ldb + c0, two, has_b, b0, b1);
  between();  // loads that do not depend on x, in flight behind the gathers
  double s0 = gs_init<BLK>(b0), s1 = gs_init<BLK>(b1);
#pragma unroll
  for (int u = 0; u < PK; ++u) {
    const double t0 = gs_acc<BLK>(s0, q.val[u], x0[u]), t1 = gs_acc<BLK>(s1, q.val[u], x1[u]);
    const bool on = (used >> u) & 1u;
    s0 = on ? t0 : s0;
    s1 = on ? t1 : s1;
  }
  if (live && gs_upd<BLK>(diag))
    mv_st2<VEC>(X + (int64_t)q.row * ldx + c0, two, gs_fin<BLK>(s0, b0, diag),
                gs_fin<BLK>(s1, b1, diag));
}

// The whole sweep in one workgroup: levels in order, __syncthreads() between them (the
// workgroup-scope visibility k_gs_block and k_gs_pipe rely on). A thread's items of a level are
// t = threadIdx.x + pass * 1024; (position, pair) advance by (1024 / KP, 1024 % KP) per pass, so
// the walk divides once. PK = 0 reads the CSR arrays through rows[] (gs_mv_row). PK = 4 or 8
// reads the level-ordered packed copy: the structure of the first pass of a level NS - 1 ahead
// is issued right after level l's gathers, which alone depend on the level before; positions
// past a level's end are clamped to its last one and not stored.
template <bool BLK, bool VEC, int PK>
__global__ __launch_bounds__(kGsBlock) void k_gs_mv_walk(
    const int32_t* __restrict__ ip, const int32_t* __restrict__ ij, const double* __restrict__ ax,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ lptr, int32_t n_levels,
    const int32_t* __restrict__ pcol, const double* __restrict__ pval,
    const double* __restrict__ pdiag, int iterations, double* X, int64_t ldx, const double* B,
    int64_t ldb, bool has_b, int k, const int32_t* done) {
  if (done && *done) return;
  const int kp = (k + 1) >> 1;
  const int32_t dq = kGsBlock / kp, dr = kGsBlock % kp;
  const int32_t pos0 = (int32_t)threadIdx.x / kp, pr0 = (int32_t)threadIdx.x % kp;
  const int c00 = 2 * pr0;
  const bool two0 = c00 + 1 < k;
  for (int it = 0; it < iterations; ++it) {
    if constexpr (PK == 0) {
      for (int32_t l = 0; l < n_levels; ++l) {
        const int32_t a = lptr[l], cnt = lptr[l + 1] - a;
        int32_t pos = pos0, pr = pr0;
        while (pos < cnt) {
          gs_mv_row<BLK, VEC>(ip, ij, ax, rows[a + pos], 2 * pr, 2 * pr + 1 < k, X, ldx, B, ldb,
                              has_b);
          pos += dq;
          pr += dr;
          if (pr >= kp) {
            pr -= kp;
            ++pos;
          }
        }
        __syncthreads();
      }
    } else {
      // first-pass position of level l (clamped into the level; l clamped into the schedule)
      auto first = [&](int32_t l) -> int64_t {
        const int32_t lc = l < n_levels ? l : n_levels - 1;
        const int32_t a = lptr[lc], cnt = lptr[lc + 1] - a;
        return a + (pos0 < cnt ? pos0 : cnt - 1);
      };
      // NS register sets rotate by unrolling, not by copies (a copy of a register with a load
      // in flight waits for it: gs.hip k_gs_ring): step l sweeps level l from S[l % NS] while
      // the structure of level l + NS - 1 goes out into the set level l - 1 used. Steps past the
      // last level sweep no row.
      constexpr int NS = PK == 4 ? 3 : 2;
      GsMvRow<PK> S[NS];
#pragma unroll
      for (int u = 0; u < NS - 1; ++u) gs_mv_struct<PK>(S[u], first(u), rows, pcol, pval);
      for (int32_t l0 = 0; l0 < n_levels; l0 += NS) {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          const int32_t l = l0 + u;
          const bool in = l < n_levels;
          const int32_t a = lptr[in ? l : n_levels - 1];
          const int32_t cnt = in ? lptr[l + 1] - a : 0;
          gs_mv_packed_row<BLK, VEC, PK>(S[u], first(l), pos0 < cnt, c00, two0, pdiag, X, ldx, B,
                                         ldb, has_b, [&]() {
                                           gs_mv_struct<PK>(S[(u + NS - 1) % NS], first(l + NS - 1),
                                                            rows, pcol, pval);
                                         });
          // the level's further passes, loaded as they come (S[u] is free until the next step
          // refills it)
          int32_t pos = pos0 + dq, pr = pr0 + dr;
          if (pr >= kp) {
            pr -= kp;
            ++pos;
          }
          while (pos < cnt) {
            gs_mv_struct<PK>(S[u], (int64_t)a + pos, rows, pcol, pval);
            gs_mv_packed_row<BLK, VEC, PK>(S[u], (int64_t)a + pos, true, 2 * pr, 2 * pr + 1 < k,
                                           pdiag, X, ldx, B, ldb, has_b, []() {});
            pos += dq;
            pr += dr;
            if (pr >= kp) {
              pr -= kp;
              ++pos;
            }
          }
          __syncthreads();
        }
      }
    }
  }
}

// MLAMG_GS_MV_WALK_ITEMS=<items> replaces both constants (A/B runs: tools/bench_block_gs.py
// measures the crossover between the walk and the per-level launches with it)
static int64_t gs_mv_walk_items(bool packed) {
  const char* e = std::getenv("MLAMG_GS_MV_WALK_ITEMS");
  if (e && e[0]) return std::atoll(e);
  return packed ? kGsMvWalkItems : kGsMvWalkItemsCsr;
}

// 0 = one launch per level, 1 = walk on the CSR arrays, 2 = walk on the packed copy
int gs_mv_path(const mlamg_gs* G, int k) {
  const int64_t kp = (k + 1) / 2;
  if (G->n_levels > 4 && (int64_t)G->max_level_rows * kp <= gs_mv_walk_items(G->pk_k > 0))
    return G->pk_k > 0 ? 2 : 1;
  return 0;
}

template <bool BLK, bool VEC>
static void launch_gs_mv(const mlamg_gs* G, int path, double* X, int64_t ldx, const double* B,
                         int64_t ldb, int k, int iterations, const int32_t* done, hipStream_t s) {
  const mlamg_csr* A = G->A;
  // a zero right-hand side: the kernels read the iterate in B's place and select +0.0
  const bool has_b = B != nullptr;
  if (!has_b) {
    B = X;
    ldb = ldx;
  }
  if (path == 0) {
    const int64_t kp = (k + 1) / 2;
    for (int it = 0; it < iterations; ++it) {
      for (int32_t l = 0; l < G->n_levels; ++l) {
        const int32_t a = G->level_ptr[l], cnt = G->level_ptr[l + 1] - a;
        hipLaunchKernelGGL((k_gs_mv_level<BLK, VEC>), dim3((unsigned)((cnt * kp + 255) / 256)),
                           dim3(256), 0, s, A->indptr, A->indices, A->data, G->rows + a, cnt, X,
                           ldx, B, ldb, has_b, k, done);
      }
    }
    return;
  }
  auto walk = [&](auto pk) {
    hipLaunchKernelGGL((k_gs_mv_walk<BLK, VEC, decltype(pk)::value>), dim3(1), dim3(kGsBlock), 0,
                       s, A->indptr, A->indices, A->data, G->rows, G->d_level_ptr, G->n_levels,
                       G->pk_col, G->pk_val, G->pk_diag, iterations, X, ldx, B, ldb, has_b, k,
                       done);
  };
  if (path == 1) walk(std::integral_constant<int, 0>());
  else if (G->pk_k == 4) walk(std::integral_constant<int, 4>());
  else walk(std::integral_constant<int, 8>());
}

static int gs_sweep_mv_one(const mlamg_gs* G, double* X, int64_t ldx, const double* B,
                           int64_t ldb, int k, int iterations, const int32_t* done,
                           hipStream_t s) {
  if (G->A->n_rows == 0 || iterations <= 0) return MLAMG_OK;
  const int path = gs_mv_path(G, k);
  // 16-byte accesses need 16-byte-aligned blocks, even leading dimensions and an even k
  const bool vec = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 &&
                   ((ldx | (B ? ldb : 0) | k) & 1) == 0;
  if (G->block) {
    if (vec) launch_gs_mv<true, true>(G, path, X, ldx, B, ldb, k, iterations, done, s);
    else launch_gs_mv<true, false>(G, path, X, ldx, B, ldb, k, iterations, done, s);
  } else {
    if (vec) launch_gs_mv<false, true>(G, path, X, ldx, B, ldb, k, iterations, done, s);
    else launch_gs_mv<false, false>(G, path, X, ldx, B, ldb, k, iterations, done, s);
  }
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// one iteration of a symmetric sweep = the forward schedule, then the backward one
int gs_sweep_mv_impl(const mlamg_gs* G, double* X, int64_t ldx, const double* B, int64_t ldb,
                     int k, int iterations, const int32_t* done, hipStream_t s) {
  if (!G->bwd) return gs_sweep_mv_one(G, X, ldx, B, ldb, k, iterations, done, s);
  for (int it = 0; it < iterations; ++it) {
    MLAMG_TRY(gs_sweep_mv_one(G, X, ldx, B, ldb, k, 1, done, s));
    MLAMG_TRY(gs_sweep_mv_one(G->bwd, X, ldx, B, ldb, k, 1, done, s));
  }
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_gs_sweep_mv(const mlamg_gs* G, double* X, int64_t ldx, const double* B, int64_t ldb,
                      int k, int iterations, void* stream) {
  MLAMG_REQUIRE(G, "G is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(k >= 1 && k <= MLAMG_MV_MAX, "k must be in [1, MLAMG_MV_MAX = 64]");
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(!B || ldb >= k, "ldb < k");
  MLAMG_REQUIRE(B != X, "B and X must differ");
  return gs_sweep_mv_impl(G, X, ldx, B, ldb, k, iterations, nullptr, S(stream));
}

int mlamg_gs_mv_path(const mlamg_gs* G, int k, int32_t* path) {
  MLAMG_REQUIRE(G, "G is NULL");
  MLAMG_REQUIRE(path, "path is NULL");
  MLAMG_REQUIRE(k >= 1 && k <= MLAMG_MV_MAX, "k must be in [1, MLAMG_MV_MAX = 64]");
  *path = gs_mv_path(G, k);
  return MLAMG_OK;
}

}  // extern "C"
