// Lexicographic Gauss-Seidel sweeps, pyamg semantics:
//   gauss_seidel (the smoother of the reference driver, ns/lib/multigrid.py:175,184):
//     for i in 0..n-1: rsum = sum_{j != i} A_ij x_j (stored order); diag = A_ii (last one);
//                      if diag != 0: x_i = (b_i - rsum) / diag
//   block_gauss_seidel with 1 x 1 blocks (the pre/post smoother and the candidate improvement of
//   pyamg's smoothed_aggregation_solver, which ns/preconditioner/PyAMG.py:94 builds; amg_core
//   block_gauss_seidel): rsum = b_i; rsum -= (0 + A_ij x_j) for j != i in stored order;
//     x_i = 0 + Dinv_i rsum, Dinv_i = pinv(A_ii) = 1 / A_ii (0 when A_ii = 0)
//   sweep 'forward' (rows 0..n-1), 'backward' (n-1..0) or 'symmetric' (forward, then backward,
//   per iteration).
// Row i reads x_j of rows swept before it after their update and the others before theirs.
// Level scheduling keeps exactly that order on the GPU: level(i) = 1 + max level(j) over rows j
// swept before i and coupled to i in either direction (a_ij or a_ji nonzero), so every row of a
// level sees final values of all earlier-coupled rows and old values of all later-coupled rows;
// rows inside a level are independent. Results are therefore bit for bit those of the sequential
// sweep.
#include "gs.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace mlamg {

template <bool BLK>
__device__ __forceinline__ void gs_row(const int32_t* __restrict__ ip,
                                       const int32_t* __restrict__ ij,
                                       const double* __restrict__ ax, int32_t i, double* x,
                                       const double* __restrict__ b) {
  double s = gs_init<BLK>(b[i]), diag = 0.0;
  for (int k = ip[i]; k < ip[i + 1]; ++k) {
    const int32_t j = ij[k];
    if (j == i) diag = ax[k];
    else s = gs_acc<BLK>(s, ax[k], x[j]);
  }
  if (BLK) diag = diag != 0.0 ? 1.0 / diag : 0.0;
  if (gs_upd<BLK>(diag)) x[i] = gs_fin<BLK>(s, b[i], diag);
}

template <bool BLK>
__global__ __launch_bounds__(256) void k_gs_level(const int32_t* __restrict__ ip,
                                                  const int32_t* __restrict__ ij,
                                                  const double* __restrict__ ax,
                                                  const int32_t* __restrict__ rows, int32_t cnt,
                                                  double* x, const double* __restrict__ b,
                                                  const int32_t* done) {
  if (done && *done) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= cnt) return;
  gs_row<BLK>(ip, ij, ax, rows[t], x, b);
}

// The whole sweep in one workgroup: levels in order, a barrier between consecutive levels
// (workgroup-scope visibility of the x updates). For operators whose levels are narrow, where
// one launch per level would make the sweep launch-bound.
template <bool BLK>
__global__ __launch_bounds__(kGsBlock) void k_gs_block(const int32_t* __restrict__ ip,
                                                       const int32_t* __restrict__ ij,
                                                       const double* __restrict__ ax,
                                                       const int32_t* __restrict__ rows,
                                                       const int32_t* __restrict__ lptr,
                                                       int32_t n_levels, int iterations, double* x,
                                                       const double* __restrict__ b,
                                                       const int32_t* done) {
  if (done && *done) return;
  for (int it = 0; it < iterations; ++it) {
    for (int32_t l = 0; l < n_levels; ++l) {
      const int32_t a = lptr[l], z = lptr[l + 1];
      for (int32_t t = a + (int32_t)threadIdx.x; t < z; t += kGsBlock) gs_row<BLK>(ip, ij, ax, rows[t], x, b);
      __syncthreads();
    }
  }
}

// One workgroup, rows with many off-diagonals (coarse Galerkin operators: 10-120 entries): LPR
// lanes per row (8, or 16 past 64 entries), EPL entries per lane, 1024 / LPR rows per pass. A row's lanes gather their entries'
// x values in parallel and leave the products (and the diagonal) in LDS in stored order; the
// row's first lane then folds them in that order — the same products, in the same order, as
// gs_row — and stores x_i. The next level's first pass (position info from the level-ordered
// `wpos` = (row, first entry, length), then its columns and values: none of it depends on x) is
// loaded while this level computes, so a level's critical path is its x gathers, the fold and
// the barrier.
constexpr int kGsWaveBlock = 1024;

template <int EPL>
struct GsWaveRow {
  int32_t row, len;
  double bi;
  int32_t col[EPL];
  double val[EPL];
};

// a position's (row, first entry, length): w.x < 0 marks no row
__device__ __forceinline__ int4 gs_wave_pos(int32_t t, int32_t z, const int4* __restrict__ wpos) {
  return t < z ? wpos[t] : make_int4(-1, 0, 0, 0);
}

// the row's b and entries from its position info
template <int LPR, int EPL>
__device__ __forceinline__ void gs_wave_entries(GsWaveRow<EPL>& r, int4 w, int lane,
                                                const int32_t* __restrict__ ij,
                                                const double* __restrict__ ax,
                                                const double* __restrict__ b) {
  const bool live = w.x >= 0;
  r.row = w.x;  // an empty row still updates (block_gauss_seidel: x_i = 0 + 0 b_i)
  r.len = w.z;
  r.bi = live ? b[w.x] : 0.0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int k = lane + e * LPR;
    const bool ok = k < w.z;
    r.col[e] = ok ? ij[w.y + k] : -1;
    r.val[e] = ok ? ax[w.y + k] : 0.0;
  }
}

template <int LPR, int EPL>
__device__ __forceinline__ void gs_wave_load(GsWaveRow<EPL>& r, int32_t t, int32_t z, int lane,
                                             const int4* __restrict__ wpos,
                                             const int32_t* __restrict__ ij,
                                             const double* __restrict__ ax,
                                             const double* __restrict__ b) {
  gs_wave_entries<LPR, EPL>(r, gs_wave_pos(t, z, wpos), lane, ij, ax, b);
}

template <int LPR, int EPL, bool BLK>
__global__ __launch_bounds__(kGsWaveBlock) void k_gs_wave(const int4* __restrict__ wpos,
                                                         const int32_t* __restrict__ ij,
                                                         const double* __restrict__ ax,
                                                         const int32_t* __restrict__ lptr,
                                                         int32_t n_levels, int iterations,
                                                         double* x, const double* __restrict__ b,
                                                         const int32_t* done) {
  constexpr int ROWS = kGsWaveBlock / LPR;  // rows per pass
  constexpr int SPAN = LPR * EPL;             // LDS slots per row
  __shared__ double pv[ROWS * SPAN];
  __shared__ int32_t pc[ROWS * SPAN];
  if (done && *done) return;
  const int tid = threadIdx.x;
  const int g = tid / LPR, lane = tid % LPR;
  double* gv = pv + g * SPAN;
  int32_t* gc = pc + g * SPAN;
  for (int it = 0; it < iterations; ++it) {
    GsWaveRow<EPL> cur, nxt;
    gs_wave_load<LPR, EPL>(cur, lptr[0] + g, lptr[1], lane, wpos, ij, ax, b);
    // positions two levels ahead, entries one level ahead (the entries need the positions)
    int4 w1 = n_levels > 1 ? gs_wave_pos(lptr[1] + g, lptr[2], wpos) : make_int4(-1, 0, 0, 0);
    int4 w2 = make_int4(-1, 0, 0, 0);
    for (int32_t l = 0; l < n_levels; ++l) {
      const int32_t a = lptr[l], z = lptr[l + 1];
      // passes over the level's rows (uniform for the workgroup: the LDS fences are per wave)
      for (int32_t t0 = a; t0 < z; t0 += ROWS) {
        if (t0 > a) gs_wave_load<LPR, EPL>(cur, t0 + g, z, lane, wpos, ij, ax, b);
        double p[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int32_t j = cur.col[e];
          const double xj = (j >= 0 && j != cur.row) ? x[j] : 0.0;
          p[e] = j == cur.row ? cur.val[e] : (BLK ? 0.0 + cur.val[e] * xj : cur.val[e] * xj);
        }
        if (t0 == a) {
          if (l + 1 < n_levels) gs_wave_entries<LPR, EPL>(nxt, w1, lane, ij, ax, b);
          if (l + 2 < n_levels) w2 = gs_wave_pos(lptr[l + 2] + g, lptr[l + 3], wpos);
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int k = lane + e * LPR;
          gv[k] = p[e];
          gc[k] = cur.col[e];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0 && cur.row >= 0) {
          double s = gs_init<BLK>(cur.bi), diag = 0.0;
          int k = 0;
          // 8 LDS reads in flight, then the 8 ordered steps
          for (; k + 8 <= cur.len; k += 8) {
            double v[8];
            int32_t c[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              v[u] = gv[k + u];
              c[u] = gc[k + u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              if (c[u] == cur.row) diag = v[u];
              else s = BLK ? s - v[u] : s + v[u];
            }
          }
          for (; k < cur.len; ++k) {
            const double v = gv[k];
            if (gc[k] == cur.row) diag = v;
            else s = BLK ? s - v : s + v;
          }
          if (BLK) diag = diag != 0.0 ? 1.0 / diag : 0.0;
          if (gs_upd<BLK>(diag)) x[cur.row] = gs_fin<BLK>(s, cur.bi, diag);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      __syncthreads();
      cur = nxt;
      w1 = w2;
    }
  }
}

// Pipelined one-workgroup sweep for narrow schedules (every level <= R * 1024 rows, every row
// <= K = 4 or 8 off-diagonals): the level-ordered structure (row id, diagonal, b, columns,
// values) of level l+1 is loaded while level l computes, so a level's critical path is only
// its x gathers (which depend on the level before), the ordered sum, the store and the barrier.
// Same products, same order, same division as gs_row: bitwise the sequential sweep.
template <int R, int K>
struct GsRows {
  int32_t row[R];
  double diag[R], bi[R];
  int32_t col[R][K];
  double val[R][K];
};

// position p's structure: independent loads only (no pointer chasing), one round trip
template <int R, int K>
__device__ __forceinline__ void gs_pipe_load(GsRows<R, K>& q, int32_t a, int32_t z,
                                             const int32_t* __restrict__ rows,
                                             const int32_t* __restrict__ pcol,
                                             const double* __restrict__ pval,
                                             const double* __restrict__ pdiag,
                                             const double* __restrict__ blvl) {
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int32_t p = a + (int32_t)threadIdx.x + u * kGsBlock;
    const bool ok = p < z;
    q.row[u] = ok ? rows[p] : -1;
    q.diag[u] = ok ? pdiag[p] : 0.0;
    q.bi[u] = ok ? blvl[p] : 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      q.col[u][k] = ok ? pcol[(int64_t)p * K + k] : -1;
      q.val[u][k] = ok ? pval[(int64_t)p * K + k] : 0.0;
    }
  }
}

template <int R, int K, bool BLK>
__global__ __launch_bounds__(kGsBlock) void k_gs_pipe(const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ lptr,
                                                      int32_t n_levels,
                                                      const int32_t* __restrict__ pcol,
                                                      const double* __restrict__ pval,
                                                      const double* __restrict__ pdiag,
                                                      const double* __restrict__ blvl,
                                                      int iterations, double* x,
                                                      const int32_t* done) {
  if (done && *done) return;
  for (int it = 0; it < iterations; ++it) {
    GsRows<R, K> cur;
    gs_pipe_load<R, K>(cur, lptr[0], lptr[1], rows, pcol, pval, pdiag, blvl);
    for (int32_t l = 0; l < n_levels; ++l) {
      // this level's x gathers first (they read the previous level's updates) ...
      double xv[R][K];
#pragma unroll
      for (int u = 0; u < R; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) xv[u][k] = cur.col[u][k] >= 0 ? x[cur.col[u][k]] : 0.0;
      // ... then the next level's structure (independent of x) in flight meanwhile
      GsRows<R, K> nxt;
      if (l + 1 < n_levels)
        gs_pipe_load<R, K>(nxt, lptr[l + 1], lptr[l + 2], rows, pcol, pval, pdiag, blvl);
#pragma unroll
      for (int u = 0; u < R; ++u) {
        if (cur.row[u] < 0) continue;
        double rsum = gs_init<BLK>(cur.bi[u]);
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (cur.col[u][k] >= 0) rsum = gs_acc<BLK>(rsum, cur.val[u][k], xv[u][k]);
        if (gs_upd<BLK>(cur.diag[u]))
          x[cur.row[u]] = gs_fin<BLK>(rsum, cur.bi[u], cur.diag[u]);
      }
      __syncthreads();
      if (l + 1 < n_levels) cur = nxt;
    }
  }
}

// Levels of 513..1024 rows with <= 4 off-diagonals (2-D five-point grids up to 1024^2): the
// pipelined walk with the x values of the last W levels in an LDS ring indexed by level-order
// position, W = the widest level distance of a coupling to an earlier level. A slot's column is
// host-classified: a row swept earlier (its updated value: the ring) or later (its old value,
// which nothing writes before the slot's own row is swept). The later-swept slots' products
// (0 + a x_old for block_gauss_seidel, a x_old for gauss_seidel: the very operation the sweep would
// do, so the same bits) are formed before the sweep by a parallel pass (k_gs_ring_prep), which also
// stores the old x of a zero-diagonal gauss_seidel row in place of its b. The sweep's loads thus
// depend on nothing the sweep computes: each level's structure goes out kGsRingSets - 1 levels
// ahead, all loads unconditional (positions past a level's end clamped to the last one and
// selected away), the level starts in LDS, and the register sets rotate by unrolling, not by
// copies (a copy of a register with a load in flight, or a branch join, makes the compiler wait
// for every outstanding load: that had put one or two memory round trips on each level's critical
// path, 2.5 us a level at 1024^2). Same products, same order, same division as gs_row.
constexpr int kGsRingSets = 6;                // levels in flight + 1
struct GsRingRow {
  int32_t pos;  // unclamped
  bool ok;      // pos inside its level
  double diag, bi;
  uint2 code;  // 4 x 16 bits: the ring slot of an earlier-swept column, kGsRingLater, kGsRingPad
  double pv[kGsRingK];
};

template <bool BLK>
__device__ __forceinline__ double gs_prod(double a, double xj) {
  return BLK ? 0.0 + a * xj : a * xj;
}
template <bool BLK>
__device__ __forceinline__ double gs_acc_prod(double s, double t) {
  return BLK ? s - t : s + t;
}

// pv[p, k] = a (earlier-swept column: multiplied in the sweep), the product with the old x
// (later-swept), 0 (pad); blvl[p] = b[row], or x[row] for a zero-diagonal gauss_seidel row
template <bool BLK>
__global__ void k_gs_ring_prep(const int32_t* __restrict__ rows, int64_t n,
                               const int32_t* __restrict__ rcol, const double* __restrict__ pval,
                               const double* __restrict__ pdiag, const double* __restrict__ b,
                               const double* __restrict__ x, double* __restrict__ pv,
                               double* __restrict__ blvl, const int32_t* done) {
  if (done && *done) return;
  const int64_t p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= n) return;
  const int32_t i = rows[p];
  blvl[p] = (!BLK && pdiag[p] == 0.0) ? x[i] : b[i];
#pragma unroll
  for (int k = 0; k < kGsRingK; ++k) {
    const int32_t c = rcol[p * kGsRingK + k];
    const double a = pval[p * kGsRingK + k];
    pv[p * kGsRingK + k] = c >= 0 ? a : (c == -1 ? 0.0 : gs_prod<BLK>(a, x[-(c + 2)]));
  }
}

__device__ __forceinline__ void gs_ring_struct(GsRingRow& q, int32_t a, int32_t z, int32_t last,
                                               const uint2* __restrict__ rcode,
                                               const double* __restrict__ pv,
                                               const double* __restrict__ pdiag,
                                               const double* __restrict__ blvl) {
  const int32_t p = a + (int32_t)threadIdx.x;
  q.ok = p < z;
  q.pos = p;
  const int64_t pc = q.ok ? p : last;
  q.diag = pdiag[pc];
  q.bi = blvl[pc];
  q.code = rcode[pc];
  const double2 v01 = *reinterpret_cast<const double2*>(pv + pc * kGsRingK);
  const double2 v23 = *reinterpret_cast<const double2*>(pv + pc * kGsRingK + 2);
  q.pv[0] = v01.x;
  q.pv[1] = v01.y;
  q.pv[2] = v23.x;
  q.pv[3] = v23.y;
}

// the row's new value into the ring and, in level order, into xl (a zero-diagonal gauss_seidel
// row's bi holds its old x: that is its value)
template <bool BLK>
__device__ __forceinline__ void gs_ring_row(const GsRingRow& q, double* ring, int32_t RM,
                                            double* __restrict__ xl) {
  const uint32_t c[4] = {q.code.x & 0xFFFFu, q.code.x >> 16, q.code.y & 0xFFFFu, q.code.y >> 16};
  double rsum = gs_init<BLK>(q.bi);
#pragma unroll
  for (int k = 0; k < kGsRingK; ++k) {
    const double r = ring[c[k] & (uint32_t)RM];
    const double t = c[k] < kGsRingLater ? gs_prod<BLK>(q.pv[k], r) : q.pv[k];
    const double u = gs_acc_prod<BLK>(rsum, t);
    rsum = c[k] != kGsRingPad ? u : rsum;
  }
  const double xi = gs_upd<BLK>(q.diag) ? gs_fin<BLK>(rsum, q.bi, q.diag) : q.bi;
  ring[q.ok ? (q.pos & RM) : RM + 1] = xi;  // slot RM + 1: the sink of the clamped lanes
  if (q.ok) xl[q.pos] = xi;
}

template <bool BLK>
__global__ __launch_bounds__(kGsBlock) void k_gs_ring(const int32_t* __restrict__ lptr,
                                                      int32_t n_levels,
                                                      const uint2* __restrict__ rcode,
                                                      const double* __restrict__ pv,
                                                      const double* __restrict__ pdiag,
                                                      const double* __restrict__ blvl,
                                                      int ring_log2, double* __restrict__ xl,
                                                      const int32_t* done) {
  extern __shared__ double ring[];  // 2^ring_log2 slots, the sink slot, then the level starts
  if (done && *done) return;
  const int32_t RM = (1 << ring_log2) - 1;
  int32_t* lp = reinterpret_cast<int32_t*>(ring + (RM + 2));
  for (int i = threadIdx.x; i <= n_levels; i += kGsBlock) lp[i] = lptr[i];
  __syncthreads();
  const int32_t nl = n_levels, last = lp[nl] - 1;
  auto lvl = [&](GsRingRow& q, int32_t l) {  // level l's structure (l >= nl: no row)
    const int32_t a = lp[l < nl ? l : nl], z = lp[l + 1 < nl ? l + 1 : nl];
    gs_ring_struct(q, a, z, last, rcode, pv, pdiag, blvl);
  };
  constexpr int NS = kGsRingSets;
  GsRingRow S[NS];
#pragma unroll
  for (int u = 0; u < NS - 1; ++u) lvl(S[u], u);
  // step l: level l + NS - 1's structure goes out (into the set level l - 1 used), level l is
  // swept; the steps past the last level sweep no row
  for (int32_t l = 0; l < nl; l += NS) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      lvl(S[(u + NS - 1) % NS], l + u + NS - 1);
      gs_ring_row<BLK>(S[u], ring, RM, xl);
      __syncthreads();
    }
  }
}

// Rows longer than 8 off-diagonals (Galerkin levels; the wave-cooperative sweep's rows) with the
// ring scheme of k_gs_ring: LPR lanes per row, each holding EPL slots of a level-ordered copy
// padded to SPAN = LPR EPL slots per position (no pointer chasing: a step's loads depend on the
// step index alone). Slot codes are fixed at setup: >= 0 the ring slot of an earlier-swept column
// at most Wr levels back, <= kGsWringFar - p an earlier-swept column further back (its value is
// read from xl at position p, two steps ahead: written at least Wr > NS levels before), or
// later-swept / diagonal / pad. The slots' values are formed before each sweep by
// k_gs_wring_prep (the later-swept products, the others' matrix values); the lanes form the
// earlier-swept products and the row's first lane folds them in stored order, as k_gs_wave does.
// A step is up to 1024 / LPR rows of one level (host table); the register sets of NS steps rotate
// by unrolling. Values go to xl in level order (one scatter after the sweep).
template <int EPL>
constexpr int gs_wring_sets() {
  return 5;
}
// four slots per lane: 512-thread workgroups (two waves per SIMD: 256 VGPRs for the five sets)
template <int EPL>
constexpr int gs_wring_threads() {
  return EPL <= 2 ? 1024 : 512;
}

template <bool BLK>
__global__ void k_gs_wring_prep(const int32_t* __restrict__ rows, int64_t n,
                                const int32_t* __restrict__ ip, const int32_t* __restrict__ ij,
                                const double* __restrict__ ax, const int32_t* __restrict__ code,
                                int span, const double* __restrict__ b,
                                const double* __restrict__ x, double* __restrict__ pv,
                                double* __restrict__ blvl, double* __restrict__ dlvl,
                                const int32_t* done) {
  if (done && *done) return;
  const int64_t p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= n) return;
  const int32_t i = rows[p], k0 = ip[i], len = ip[i + 1] - k0;
  double diag = 0.0;
  for (int k = 0; k < len; ++k) {
    const int32_t c = code[p * span + k];
    const double a = ax[k0 + k];
    pv[p * span + k] = c == kGsWringLater ? gs_prod<BLK>(a, x[ij[k0 + k]]) : a;
    if (c == kGsWringDiag) diag = a;  // the last stored diagonal entry counts
  }
  blvl[p] = (!BLK && diag == 0.0) ? x[i] : b[i];
  dlvl[p] = BLK ? (diag != 0.0 ? 1.0 / diag : 0.0) : diag;
}

template <int EPL>
struct GsWringRow {
  int32_t pos, len;
  bool ok;
  double bi, dg;
  int32_t code[EPL];
  double pv[EPL], xf[EPL];
};

template <int LPR, int EPL, bool BLK>
__global__ __launch_bounds__(gs_wring_threads<EPL>()) void k_gs_wring(const int2* __restrict__ steps, int32_t n_steps,
                                                   int32_t last, const int32_t* __restrict__ code,
                                                   const double* __restrict__ pv,
                                                   const int32_t* __restrict__ plen,
                                                   const double* __restrict__ blvl,
                                                   const double* __restrict__ dlvl,
                                                   int ring_log2, double* xl,
                                                   const int32_t* done) {
  constexpr int TPB = gs_wring_threads<EPL>();
  constexpr int ROWS = TPB / LPR, SPAN = LPR * EPL, NS = gs_wring_sets<EPL>();
  extern __shared__ double lds[];  // ring (2^ring_log2 + 2) | products | diag flags | steps
  if (done && *done) return;
  const int32_t RM = (1 << ring_log2) - 1;
  double* ring = lds;
  double* gv = ring + (RM + 3);
  uint16_t* gc = reinterpret_cast<uint16_t*>(gv + ROWS * SPAN);
  int2* st = reinterpret_cast<int2*>(gc + ROWS * SPAN + 4);
  for (int i = threadIdx.x; i < n_steps; i += TPB) st[i] = steps[i];
  __syncthreads();
  const int g = threadIdx.x / LPR, lane = threadIdx.x % LPR;
  auto load = [&](GsWringRow<EPL>& q, int32_t t) {  // step t's structure (t >= n_steps: none)
    const int2 d = st[t < n_steps ? t : n_steps - 1];
    q.ok = t < n_steps && g < d.y;
    q.pos = d.x + g;
    const int64_t pc = q.ok ? q.pos : last;
    q.len = plen[pc];
    q.bi = blvl[pc];
    q.dg = dlvl[pc];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      q.code[e] = code[pc * SPAN + lane + e * LPR];
      q.pv[e] = pv[pc * SPAN + lane + e * LPR];
    }
  };
  auto gather = [&](GsWringRow<EPL>& q) {  // the far columns' values (needs the codes)
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int32_t c = q.code[e];
      q.xf[e] = xl[c <= kGsWringFar ? kGsWringFar - c : 0];
    }
  };
  double* myv = gv + g * SPAN;
  uint16_t* myc = gc + g * SPAN;
  auto sweep = [&](const GsWringRow<EPL>& q) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int32_t c = q.code[e];
      const double r = ring[c & RM];
      const bool near = c >= 0, far = c <= kGsWringFar;
      myv[lane + e * LPR] = (near || far) ? gs_prod<BLK>(q.pv[e], near ? r : q.xf[e]) : q.pv[e];
      myc[lane + e * LPR] = (uint16_t)(c == kGsWringDiag);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0 && q.ok) {
      double sum = gs_init<BLK>(q.bi);
      int k = 0;
      for (; k + 8 <= q.len; k += 8) {  // 8 LDS reads in flight, then the 8 ordered steps
        double v[8];
        uint32_t dflag[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          v[u] = myv[k + u];
          dflag[u] = myc[k + u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (!dflag[u]) sum = gs_acc_prod<BLK>(sum, v[u]);
      }
      for (; k < q.len; ++k)
        if (!myc[k]) sum = gs_acc_prod<BLK>(sum, myv[k]);
      const double xi = gs_upd<BLK>(q.dg) ? gs_fin<BLK>(sum, q.bi, q.dg) : q.bi;
      ring[q.pos & RM] = xi;
      xl[q.pos] = xi;
    }
    __syncthreads();
  };
  // step t: step t + NS - 1's structure and step t + NS - 3's far values go out, step t is swept
  GsWringRow<EPL> S[NS];
#pragma unroll
  for (int u = 0; u < NS - 1; ++u) load(S[u], u);
  gather(S[0]);
  gather(S[1]);
  for (int32_t t = 0; t < n_steps; t += NS) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      load(S[(u + NS - 1) % NS], t + u + NS - 1);
      gather(S[(u + 2) % NS]);
      sweep(S[u]);
    }
  }
}

// Small systems (n <= kGsLdsMax): the same pipelined walk with x held in LDS for the whole sweep
// (x loaded once, written back once): a level's gathers and its updates are LDS accesses, so a
// level costs an LDS round trip and a barrier instead of a global-memory round trip.
template <int K, bool BLK>
__global__ __launch_bounds__(kGsBlock) void k_gs_lds(const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ lptr,
                                                     int32_t n_levels, int64_t n,
                                                     const int32_t* __restrict__ pcol,
                                                     const double* __restrict__ pval,
                                                     const double* __restrict__ pdiag,
                                                     const double* __restrict__ blvl,
                                                     int iterations, double* x,
                                                     const int32_t* done) {
  extern __shared__ double xs[];
  if (done && *done) return;
  for (int64_t i = threadIdx.x; i < n; i += kGsBlock) xs[i] = x[i];
  __syncthreads();
  for (int it = 0; it < iterations; ++it) {
    GsRows<1, K> cur;
    gs_pipe_load<1, K>(cur, lptr[0], lptr[1], rows, pcol, pval, pdiag, blvl);
    for (int32_t l = 0; l < n_levels; ++l) {
      GsRows<1, K> nxt;
      if (l + 1 < n_levels)
        gs_pipe_load<1, K>(nxt, lptr[l + 1], lptr[l + 2], rows, pcol, pval, pdiag, blvl);
      if (cur.row[0] >= 0) {
        double xv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) xv[k] = cur.col[0][k] >= 0 ? xs[cur.col[0][k]] : 0.0;
        double rsum = gs_init<BLK>(cur.bi[0]);
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (cur.col[0][k] >= 0) rsum = gs_acc<BLK>(rsum, cur.val[0][k], xv[k]);
        if (gs_upd<BLK>(cur.diag[0])) xs[cur.row[0]] = gs_fin<BLK>(rsum, cur.bi[0], cur.diag[0]);
      }
      __syncthreads();
      if (l + 1 < n_levels) cur = nxt;
    }
  }
  for (int64_t i = threadIdx.x; i < n; i += kGsBlock) x[i] = xs[i];
}

// Windowed one-wave sweep for levels of <= 64 * RW rows: wave 0 walks the levels with x held by
// level-order position in an LDS ring (a level's rows read positions at most W levels away, so
// levels [l - W, l + W] are all a step needs); the 7 other waves meanwhile stage the next chunk
// of levels into the other buffer: the structure (values, columns as ring slots, diagonal, b,
// row id) and the old x of the levels entering the window, read from xl, a level-ordered copy of
// x (one independent load per position instead of rows[p] then x[rows[p]]), every load of a
// thread's positions issued before its first LDS store. Consecutive levels need only a wavefront
// fence; a chunk ends with a workgroup barrier.
// Pads point at the ring's zero slot (+0.0 products: the sum starts at +0.0 and never becomes
// -0.0, so bitwise neutral); a zero-diagonal row is left alone, as the sequential sweep does (its
// quotient goes to the sink slot). Updated values go to the ring and to xl (copied back to x by
// one coalesced pass after the launch: no scattered stores in the sweep). Same products,
// order and division: bitwise gs_row.
constexpr int kGsWinBlock = 512;
#ifndef MLAMG_GSWIN_LAB  // timing variants (tools/gs_win_lab.py): 1 = no sweep, 2 = no staging
#define MLAMG_GSWIN_LAB 0
#endif
constexpr int kGsWinStageU = 4;  // positions per staging thread with all loads in flight

template <int KM>
struct WinBuf {
  double* v;
  double* d;
  double* b;
  int32_t* l;
  uint16_t* c;
  int32_t* h;
  __device__ WinBuf(char* base, int cap) {
    char* p = base + 16;
    h = reinterpret_cast<int32_t*>(base);
    v = reinterpret_cast<double*>(p);
    p += win_a16(8 * (int64_t)(cap + 1) * KM);
    d = reinterpret_cast<double*>(p);
    p += win_a16(8 * (int64_t)(cap + 1));
    b = reinterpret_cast<double*>(p);
    p += win_a16(8 * (int64_t)(cap + 1));
    l = reinterpret_cast<int32_t*>(p);
    p += win_a16(4 * (int64_t)(cap + 2));
    c = reinterpret_cast<uint16_t*>(p);
  }
};

template <int KM>
struct WinCols {  // KM uint16 slots: one 8-byte (KM 4) or 16-byte (KM 8) LDS access
  typedef typename std::conditional<KM == 4, uint2, uint4>::type T;
};

template <int KM, int RW, int CW, bool BLK>
__global__ __launch_bounds__(kGsWinBlock) void k_gs_win(const int4* __restrict__ cdesc,
                                                     const int32_t* __restrict__ wlev,
                                                     int32_t nchunks,
                                                     const int32_t* __restrict__ wcol,
                                                     const double* __restrict__ pval,
                                                     const double* __restrict__ pdiag,
                                                     const double* __restrict__ blvl,
                                                     int ring_log2, int cap,
                                                     int iterations, double* xl,
                                                     const int32_t* done) {
  extern __shared__ double lds[];
  if (done && *done) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int RS = 1 << ring_log2, RM = RS - 1;
  double* ring = lds;  // RS slots + the zero slot (RS) + the sink slot (RS + 1)
  // the sweeping waves' level counters (CW > 1), then the staging buffers
  int32_t* flags = reinterpret_cast<int32_t*>(lds + RS + 2);
  char* bufs = reinterpret_cast<char*>(lds + ((RS + 4 + 1) & ~1));
  if (tid < 4) flags[tid] = 0;
  int seq = 0;
  const int64_t bb = win_buf_bytes(cap, KM);
  if (tid == 0) ring[RS] = 0.0;
  typedef typename WinCols<KM>::T CT;
  auto stage = [&](int ch, char* base, int t0, int nt) {
    WinBuf<KM> w(base, cap);
    // the chunk's plan (host-built): levels, first position and count, the old-x range entering
    // the window (levels [l0 + W, l1 + W) clipped; chunk 0: [0, l1 + W)) and its level starts
    const int4 c0 = cdesc[2 * ch], c1 = cdesc[2 * ch + 1];
    const int nl = c0.x, P0 = c0.y, cnt = c0.z, X0 = c0.w, xcnt = c1.x, woff = c1.y;
    if (t0 == 0) {
      w.h[0] = nl;
      w.h[1] = P0;
      w.h[2] = cnt;
    }
    const int tot = max(cnt + 1, xcnt);
    for (int q0 = t0; q0 < tot; q0 += nt * kGsWinStageU) {
      double v[kGsWinStageU][KM], d[kGsWinStageU], bv[kGsWinStageU], xo[kGsWinStageU];
      int32_t c[kGsWinStageU][KM], ls[kGsWinStageU];
#pragma unroll
      for (int u = 0; u < kGsWinStageU; ++u) {
        const int q = q0 + u * nt;
        ls[u] = wlev[woff + min(q, nl)];
        const bool in = q < cnt;
        const int64_t pp = in ? (int64_t)(P0 + q) : 0;
#pragma unroll
        for (int k = 0; k < KM; k += 4) {
          const int4 c4 = *reinterpret_cast<const int4*>(wcol + pp * KM + k);
          c[u][k] = c4.x;
          c[u][k + 1] = c4.y;
          c[u][k + 2] = c4.z;
          c[u][k + 3] = c4.w;
        }
#pragma unroll
        for (int k = 0; k < KM; k += 2) {
          const double2 v2 = *reinterpret_cast<const double2*>(pval + pp * KM + k);
          v[u][k] = v2.x;
          v[u][k + 1] = v2.y;
        }
        d[u] = pdiag[pp];
        bv[u] = blvl[pp];
        // written by wave 0 in the previous sweep of this launch: past L1
        xo[u] = q < xcnt ? __hip_atomic_load(xl + X0 + q, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)
                         : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kGsWinStageU; ++u) {
        const int q = q0 + u * nt;
        if (q <= cnt) {
          const bool dummy = q == cnt;  // lanes past a level's end: zero slots, sink target
          uint16_t cs[KM];
#pragma unroll
          for (int k = 0; k < KM; ++k)
            cs[k] = (uint16_t)(!dummy && c[u][k] >= 0 ? (c[u][k] & RM) : RS);
          *reinterpret_cast<CT*>(w.c + (int64_t)q * KM) = *reinterpret_cast<const CT*>(cs);
#pragma unroll
          for (int k = 0; k < KM; k += 2) {
            double2 v2;
            v2.x = dummy ? 0.0 : v[u][k];
            v2.y = dummy ? 0.0 : v[u][k + 1];
            *reinterpret_cast<double2*>(w.v + (int64_t)q * KM + k) = v2;
          }
          w.d[q] = dummy ? 0.0 : d[u];
          w.b[q] = dummy ? 0.0 : bv[u];
        }
        if (q < xcnt) ring[(X0 + q) & RM] = xo[u];
        if (q <= nl) w.l[q] = ls[u];
      }
    }
  };
  for (int it = 0; it < iterations; ++it) {
    stage(0, bufs, tid, kGsWinBlock);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
      char* cur = bufs + (MLAMG_GSWIN_LAB == 2 ? 0 : (ch & 1) * bb);
      if (tid < 64 * CW && MLAMG_GSWIN_LAB != 1) {
        const WinBuf<KM> w(cur, cap);
        const int nl = w.h[0], P0 = w.h[1], cnt = w.h[2];
        int c[RW][KM], p[RW];
        double v[RW][KM], d[RW], bv[RW];
        auto load = [&](int l, int (&cc)[RW][KM], double (&vv)[RW][KM], double* dd, double* bq,
                        int* pq) {
          const int a = w.l[l], z = w.l[l + 1];
#pragma unroll
          for (int u = 0; u < RW; ++u) {
            const int q0 = a + lane + 64 * (wv + CW * u);
            const int q = q0 < z ? q0 : cnt;
            const CT c4 = *reinterpret_cast<const CT*>(w.c + (int64_t)q * KM);
            const uint16_t* cs = reinterpret_cast<const uint16_t*>(&c4);
#pragma unroll
            for (int k = 0; k < KM; ++k) cc[u][k] = cs[k];
#pragma unroll
            for (int k = 0; k < KM; k += 2) {
              const double2 v2 = *reinterpret_cast<const double2*>(w.v + (int64_t)q * KM + k);
              vv[u][k] = v2.x;
              vv[u][k + 1] = v2.y;
            }
            dd[u] = w.d[q];
            bq[u] = w.b[q];
            pq[u] = q;
          }
        };
        load(0, c, v, d, bv, p);
        #pragma unroll 1
        for (int l = 0; l < nl; ++l) {
          double g[RW][KM];
#pragma unroll
          for (int u = 0; u < RW; ++u)
#pragma unroll
            for (int k = 0; k < KM; ++k) g[u][k] = ring[c[u][k]];
          int c2[RW][KM], p2[RW];
          double v2[RW][KM], d2[RW], bv2[RW];
          load(l + 1 < nl ? l + 1 : l, c2, v2, d2, bv2, p2);
          // the RW rows' sums and divisions first, as one block (their dependency chains
          // interleave), then the stores
          double xi[RW];
#pragma unroll
          for (int u = 0; u < RW; ++u) {
            double y = gs_init<BLK>(bv[u]);
#pragma unroll
            for (int k = 0; k < KM; ++k) y = gs_acc<BLK>(y, v[u][k], g[u][k]);
            xi[u] = gs_fin<BLK>(y, bv[u], d[u]);
          }
          // the dummy, and a zero-diagonal row of gauss_seidel: left alone (the sink slot)
          bool up[RW];
#pragma unroll
          for (int u = 0; u < RW; ++u) up[u] = p[u] != cnt && gs_upd<BLK>(d[u]);
#pragma unroll
          for (int u = 0; u < RW; ++u) ring[up[u] ? ((P0 + p[u]) & RM) : RS + 1] = xi[u];
#pragma unroll
          for (int u = 0; u < RW; ++u)
            if (up[u]) xl[P0 + p[u]] = xi[u];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          if (CW > 1) {
            // the level's other sweeping waves: a wave's LDS operations complete in issue
            // order, so a counter stored after the ring stores is seen after them; the spin
            // reads all counters until each has reached this level
            ++seq;
            asm volatile("" ::: "memory");
            if (lane == 0) *reinterpret_cast<volatile int32_t*>(flags + wv) = seq;
            for (;;) {
              bool ok = true;
#pragma unroll
              for (int w2 = 0; w2 < CW; ++w2)
                ok = ok && *reinterpret_cast<volatile int32_t*>(flags + w2) >= seq;
              if (ok) break;
            }
            asm volatile("" ::: "memory");
          }
#pragma unroll
          for (int u = 0; u < RW; ++u) {
#pragma unroll
            for (int k = 0; k < KM; ++k) {
              c[u][k] = c2[u][k];
              v[u][k] = v2[u][k];
            }
            d[u] = d2[u];
            bv[u] = bv2[u];
            p[u] = p2[u];
          }
        }
      } else if (tid >= 64 * CW && MLAMG_GSWIN_LAB != 2 && ch + 1 < nchunks) {
        stage(ch + 1, bufs + ((ch + 1) & 1) * bb, tid - 64 * CW, kGsWinBlock - 64 * CW);
      }
      __syncthreads();
    }
    __threadfence();  // this sweep's xl stores before the next sweep's window loads
    __syncthreads();
  }
}

__global__ void k_gs_b_level(const int32_t* __restrict__ rows, int64_t n,
                             const double* __restrict__ b, double* __restrict__ blvl,
                             const int32_t* done) {
  if (done && *done) return;
  const int64_t p = blockIdx.x * 256ll + threadIdx.x;
  if (p < n) blvl[p] = b[rows[p]];
}

// R = 1, n <= kGsLdsMax (PIPE_LDS): x held in LDS for the whole sweep
template <int R, int K, bool BLK>
static void launch_gs_pipe(const mlamg_gs* G, double* x, const double* b, int iterations,
                           const int32_t* done, hipStream_t s) {
  const int64_t n = G->A->n_rows;
  hipLaunchKernelGGL(k_gs_b_level, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, G->rows,
                     n, b, G->b_lvl, done);
  if (G->path == kGsPathPipeLds) {
    hipLaunchKernelGGL((k_gs_lds<K, BLK>), dim3(1), dim3(kGsBlock), sizeof(double) * n, s, G->rows,
                       G->d_level_ptr, G->n_levels, n, G->pk_col, G->pk_val, G->pk_diag,
                       G->b_lvl, iterations, x, done);
    return;
  }
  hipLaunchKernelGGL((k_gs_pipe<R, K, BLK>), dim3(1), dim3(kGsBlock), 0, s, G->rows, G->d_level_ptr,
                     G->n_levels, G->pk_col, G->pk_val, G->pk_diag, G->b_lvl, iterations, x,
                     done);
}

// x <- xl after the window sweeps (rows in level order: coalesced reads of xl; a zero-diagonal
// row's xl still holds its old x)
__global__ void k_gs_win_post(const int32_t* __restrict__ rows, int64_t n,
                              const double* __restrict__ xl, double* __restrict__ x,
                              const int32_t* done) {
  if (done && *done) return;
  const int64_t p = blockIdx.x * 256ll + threadIdx.x;
  if (p < n) x[rows[p]] = xl[p];
}

__global__ void k_gs_win_prep(const int32_t* __restrict__ rows, int64_t n,
                              const double* __restrict__ b, double* __restrict__ blvl,
                              const double* __restrict__ x, double* __restrict__ xl,
                              const int32_t* done) {
  if (done && *done) return;
  const int64_t p = blockIdx.x * 256ll + threadIdx.x;
  if (p < n) {
    const int32_t i = rows[p];
    blvl[p] = b[i];
    xl[p] = x[i];
  }
}

template <int KM, int RW, int CW, bool BLK>
static void launch_gs_win(const mlamg_gs* G, double* x, const double* b, int iterations,
                          const int32_t* done, hipStream_t s) {
  const int64_t n = G->A->n_rows;
  hipLaunchKernelGGL(k_gs_win_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, G->rows,
                     n, b, G->b_lvl, x, G->win_xl, done);
  hipLaunchKernelGGL((k_gs_win<KM, RW, CW, BLK>), dim3(1), dim3(kGsWinBlock), G->win_lds, s,
                     reinterpret_cast<const int4*>(G->d_clev), G->d_clev + 8 * G->n_chunks,
                     G->n_chunks, G->wcol, G->pk_val, G->pk_diag, G->b_lvl, G->ring_log2,
                     G->win_cap, iterations, G->win_xl, done);
  hipLaunchKernelGGL(k_gs_win_post, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, G->rows,
                     n, G->win_xl, x, done);
}

int64_t gs_rows(const mlamg_gs* G) { return G->A->n_rows; }

using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;
using I4 = std::integral_constant<int, 4>;
using I8 = std::integral_constant<int, 8>;
using I16 = std::integral_constant<int, 16>;

// the kernel is the plan's (G->path, gs_plan.cpp); here only its template instance is chosen
template <bool BLK>
static int gs_sweep_one(const mlamg_gs* G, double* x, const double* b, int iterations,
                        const int32_t* done, hipStream_t s) {
  const mlamg_csr* A = G->A;
  const int64_t n = A->n_rows;
  if (n == 0 || iterations <= 0) return MLAMG_OK;
  const unsigned nb = (unsigned)((n + 255) / 256);
  switch (G->path) {
    case kGsPathWindow: {
      // win_rw = 64-row slots per level: up to 4 sweeping waves, then 2 rows per lane
      auto go = [&](auto km) {
        constexpr int KM = decltype(km)::value;
        switch (G->win_rw) {
          case 1: launch_gs_win<KM, 1, 1, BLK>(G, x, b, iterations, done, s); break;
          case 2: launch_gs_win<KM, 1, 2, BLK>(G, x, b, iterations, done, s); break;
          case 3: launch_gs_win<KM, 1, 3, BLK>(G, x, b, iterations, done, s); break;
          case 4: launch_gs_win<KM, 1, 4, BLK>(G, x, b, iterations, done, s); break;
          default: launch_gs_win<KM, 2, 4, BLK>(G, x, b, iterations, done, s); break;
        }
      };
      if (G->pk_k == 4) go(I4());
      else go(I8());
      break;
    }
    case kGsPathRing:
      // one sweep per launch pair: the products of the old values are formed before each
      for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL((k_gs_ring_prep<BLK>), dim3(nb), dim3(256), 0, s, G->rows, n, G->rcol,
                           G->pk_val, G->pk_diag, b, x, G->rpv, G->b_lvl, done);
        hipLaunchKernelGGL((k_gs_ring<BLK>), dim3(1), dim3(kGsBlock), G->ring_lds, s,
                           G->d_level_ptr, G->n_levels, reinterpret_cast<const uint2*>(G->rcode),
                           G->rpv, G->pk_diag, G->b_lvl, G->ring_log2_r, G->rxl, done);
        // the level-ordered values back to x (coalesced stores in the sweep, one scatter here)
        hipLaunchKernelGGL(k_gs_win_post, dim3(nb), dim3(256), 0, s, G->rows, n, G->rxl, x, done);
      }
      break;
    case kGsPathPipe:
    case kGsPathPipeLds: {
      const bool one = G->max_level_rows <= kGsBlock;  // rows per thread R = 1, else 2
      if (G->pk_k == 4) {
        if (one) launch_gs_pipe<1, 4, BLK>(G, x, b, iterations, done, s);
        else launch_gs_pipe<2, 4, BLK>(G, x, b, iterations, done, s);
      } else {
        if (one) launch_gs_pipe<1, 8, BLK>(G, x, b, iterations, done, s);
        else launch_gs_pipe<2, 8, BLK>(G, x, b, iterations, done, s);
      }
      break;
    }
    case kGsPathWring: {
      const int span = G->wr_lpr * G->wr_epl;
      auto go = [&](auto l, auto e) {
        hipLaunchKernelGGL((k_gs_wring<decltype(l)::value, decltype(e)::value, BLK>), dim3(1),
                           dim3(gs_wring_threads<decltype(e)::value>()), G->wr_lds, s, G->wr_st, G->wr_steps, (int32_t)(n - 1),
                           G->wr_code, G->wr_pv, G->wr_len, G->b_lvl, G->wr_d, G->wr_log2, G->rxl,
                           done);
      };
      for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL((k_gs_wring_prep<BLK>), dim3(nb), dim3(256), 0, s, G->rows, n,
                           A->indptr, A->indices, A->data, G->wr_code, span, b, x, G->wr_pv,
                           G->b_lvl, G->wr_d, done);
        if (G->wr_epl == 2) {
          if (G->wr_lpr == 8) go(I8(), I2());
          else go(I16(), I2());
        } else {
          if (G->wr_lpr == 8) go(I8(), I4());
          else go(I16(), I4());
        }
        hipLaunchKernelGGL(k_gs_win_post, dim3(nb), dim3(256), 0, s, G->rows, n, G->rxl, x, done);
      }
      break;
    }
    case kGsPathWave: {
      auto go = [&](auto l, auto e) {
        hipLaunchKernelGGL((k_gs_wave<decltype(l)::value, decltype(e)::value, BLK>), dim3(1),
                           dim3(kGsWaveBlock), 0, s, reinterpret_cast<const int4*>(G->wpos),
                           A->indices, A->data, G->d_level_ptr, G->n_levels, iterations, x, b,
                           done);
      };
      auto lanes = [&](auto l) {
        switch (G->wave_epl) {
          case 1: go(l, I1()); break;
          case 2: go(l, I2()); break;
          case 4: go(l, I4()); break;
          default: go(l, I8()); break;
        }
      };
      if (G->wave_lpr == 8) lanes(I8());
      else lanes(I16());
      break;
    }
    case kGsPathWorkgroup:
      // one row per thread per level; wider levels go one launch per level over the whole chip
      hipLaunchKernelGGL(k_gs_block<BLK>, dim3(1), dim3(kGsBlock), 0, s, A->indptr, A->indices, A->data,
                         G->rows, G->d_level_ptr, G->n_levels, iterations, x, b, done);
      break;
    case kGsPathLevels:
      for (int it = 0; it < iterations; ++it) {
        for (int32_t l = 0; l < G->n_levels; ++l) {
          const int32_t a = G->level_ptr[l], cnt = G->level_ptr[l + 1] - a;
          hipLaunchKernelGGL(k_gs_level<BLK>, dim3((cnt + 255) / 256), dim3(256), 0, s, A->indptr,
                             A->indices, A->data, G->rows + a, cnt, x, b, done);
        }
      }
      break;
  }
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// one iteration of a symmetric sweep = the forward schedule, then the backward one
int gs_sweep_impl(const mlamg_gs* G, double* x, const double* b, int iterations,
                  const int32_t* done, hipStream_t s) {
  auto one = [&](const mlamg_gs* H, int it) {
    return H->block ? gs_sweep_one<true>(H, x, b, it, done, s)
                    : gs_sweep_one<false>(H, x, b, it, done, s);
  };
  if (!G->bwd) return one(G, iterations);
  for (int it = 0; it < iterations; ++it) {
    MLAMG_TRY(one(G, 1));
    MLAMG_TRY(one(G->bwd, 1));
  }
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

static_assert(sizeof(GsStep) == sizeof(int2) && offsetof(GsStep, first) == offsetof(int2, x) &&
                  offsetof(GsStep, rows) == offsetof(int2, y),
              "k_gs_wring reads the plan's steps as int2");

// frees the handle's device buffers from owned[from] on
static void gs_release(mlamg_gs* G, size_t from) {
  for (size_t i = from; i < G->owned.size(); ++i) {
    (void)hipFree(*G->owned[i]);
    *G->owned[i] = nullptr;
  }
  G->owned.resize(from);
}

// Every device buffer of a handle is made here: `count` elements (at least one) for the handle's
// field, filled from `src` unless nullptr, owned by the handle from then on. After a failure rc
// is set and further calls do nothing.
struct GsUpload {
  mlamg_gs* G;
  int rc = MLAMG_OK;
  template <class T, class U = T>
  void put(T** field, size_t count, const U* src = nullptr) {
    static_assert(sizeof(T) == sizeof(U), "element sizes differ");
    if (rc != MLAMG_OK) return;
    if (hipMalloc(field, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) {
      *field = nullptr;
      set_error("gs_create: hipMalloc failed");
      rc = MLAMG_ENOMEM;
      return;
    }
    G->owned.push_back(reinterpret_cast<void**>(field));
    if (src && count &&
        hipMemcpy(*field, src, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) {
      set_error("gs_create: hipMemcpy failed");
      rc = MLAMG_EHIP;
    }
  }
};

// The device side of a plan. rows and the level starts are mandatory; a layout that cannot be
// allocated or copied gives back what it had got and is dropped from the plan's candidates, and
// the path is chosen among what is left.
static int gs_upload(mlamg_gs* G, GsPlan& P) {
  const size_t n = (size_t)P.n;
  GsUpload up{G};
  G->level_ptr = P.level_ptr;
  up.put(&G->rows, n, P.rows.data());
  up.put(&G->d_level_ptr, P.level_ptr.size(), P.level_ptr.data());
  if (up.rc != MLAMG_OK) return up.rc;
  auto optional = [&](bool& have, auto&& layout) {
    if (!have) return;
    const size_t mark = G->owned.size();
    layout();
    if (up.rc == MLAMG_OK) return;
    gs_release(G, mark);
    up.rc = MLAMG_OK;
    have = false;
  };
  optional(P.packed, [&] {
    up.put(&G->pk_col, P.pcol.size(), P.pcol.data());
    up.put(&G->pk_val, P.pval.size(), P.pval.data());
    up.put(&G->pk_diag, n, P.pdiag.data());
    up.put(&G->b_lvl, n);
  });
  if (P.packed) G->pk_k = P.K;
  else P.window = P.ring = false;
  optional(P.window, [&] {
    up.put(&G->wcol, P.wcol.size(), P.wcol.data());
    up.put(&G->d_clev, P.clev.size(), P.clev.data());
    up.put(&G->win_xl, n);
  });
  optional(P.ring, [&] {
    up.put(&G->rcol, P.rcol.size(), P.rcol.data());
    up.put(&G->rcode, P.rcode.size(), P.rcode.data());
    up.put(&G->rpv, P.rcol.size());
    up.put(&G->rxl, n);
  });
  optional(P.wave, [&] { up.put(&G->wpos, P.wpos.size(), P.wpos.data()); });
  optional(P.wring, [&] {
    up.put(&G->wr_pv, P.wr_code.size());  // pads stay 0: zeroed while the copies below run
    if (up.rc == MLAMG_OK &&
        hipMemset(G->wr_pv, 0, sizeof(double) * P.wr_code.size()) != hipSuccess)
      up.rc = MLAMG_EHIP;
    up.put(&G->wr_code, P.wr_code.size(), P.wr_code.data());
    up.put(&G->wr_len, n, P.wr_len.data());
    up.put(&G->wr_st, P.wr_st.size(), P.wr_st.data());
    up.put(&G->wr_d, n);
    up.put(&G->rxl, n);
    up.put(&G->b_lvl, n);
  });
  P.path = gs_select_path(P);
  static_cast<GsScalars&>(*G) = P;
  return MLAMG_OK;
}

// one sweep direction's schedule and layouts into a new handle (*out owns it, also on failure)
static int gs_build(const mlamg_csr* A, bool backward, bool block, const GsKnobs& knobs,
                    mlamg_gs** out, hipStream_t s) {
  mlamg_gs* G = *out = new mlamg_gs();
  G->A = A;
  G->block = block;
  const int64_t n = A->n_rows;
  // MLAMG_TIMING=1: host phase times of the schedule analysis on stderr
  static const bool timing = std::getenv("MLAMG_TIMING") != nullptr;
  auto t_prev = std::chrono::steady_clock::now();
  auto phase = [&](const char* name) {
    if (!timing) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[gs_create] %s %.3f ms\n", name,
                 std::chrono::duration<double, std::milli>(t - t_prev).count());
    t_prev = t;
  };
  std::vector<int32_t> ip(n + 1), ij(A->nnz);
  MLAMG_HIP(hipMemcpyAsync(ip.data(), A->indptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, s));
  if (A->nnz)
    MLAMG_HIP(hipMemcpyAsync(ij.data(), A->indices, sizeof(int32_t) * A->nnz, hipMemcpyDeviceToHost, s));
  MLAMG_HIP(hipStreamSynchronize(s));
  phase("copy_in");
  GsPlan P;
  gs_plan_structure(ip.data(), ij.data(), n, backward, P);
  phase("levels");
  {
    std::vector<double> ax;
    if (P.packed) {  // only the packed copy holds values: other schedules leave A's on the device
      ax.resize(A->nnz);
      if (A->nnz)
        MLAMG_HIP(hipMemcpy(ax.data(), A->data, sizeof(double) * A->nnz, hipMemcpyDeviceToHost));
    }
    gs_plan_layouts(ip.data(), ij.data(), ax.data(), block, knobs, P);
  }
  phase("layouts");
  MLAMG_TRY(gs_upload(G, P));
  phase("upload");
  return MLAMG_OK;
}

extern "C" {

int mlamg_gs_create_ex(const mlamg_csr* A, int sweep, int block, mlamg_gs** out, void* stream) {
  MLAMG_REQUIRE(A && out, "NULL argument");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "square matrix required");
  MLAMG_REQUIRE(sweep >= 0 && sweep <= 2, "sweep must be 0 forward, 1 backward, 2 symmetric");
  MLAMG_REQUIRE(block == 0 || block == 1, "block must be 0 or 1");
  hipStream_t s = S(stream);
  const GsKnobs knobs = GsKnobs::from_env();
  mlamg_gs* G = nullptr;  // a failed build leaves its half-built handle here, or in G->bwd
  int rc = gs_build(A, sweep == 1, block == 1, knobs, &G, s);
  if (rc == MLAMG_OK && sweep == 2) rc = gs_build(A, true, block == 1, knobs, &G->bwd, s);
  if (rc != MLAMG_OK) {
    mlamg_gs_destroy(G);
    return rc;
  }
  *out = G;
  return MLAMG_OK;
}

int mlamg_gs_create(const mlamg_csr* A, mlamg_gs** out, void* stream) {
  return mlamg_gs_create_ex(A, 0, 0, out, stream);
}

int mlamg_gs_destroy(mlamg_gs* G) {
  if (G) {
    if (G->bwd) mlamg_gs_destroy(G->bwd);
    gs_release(G, 0);
    delete G;
  }
  return MLAMG_OK;
}

int mlamg_gs_levels(const mlamg_gs* G, int32_t* n_levels) {
  MLAMG_REQUIRE(G && n_levels, "NULL argument");
  *n_levels = G->n_levels;
  return MLAMG_OK;
}

int mlamg_gs_path(const mlamg_gs* G, int which, int32_t* path) {
  MLAMG_REQUIRE(G, "G is NULL");
  MLAMG_REQUIRE(path, "path is NULL");
  MLAMG_REQUIRE(which == 0 || which == 1, "which must be 0 (own schedule) or 1 (backward half)");
  MLAMG_REQUIRE(which == 0 || G->bwd, "which = 1 needs a symmetric handle");
  *path = which ? G->bwd->path : G->path;
  return MLAMG_OK;
}

int mlamg_gs_sweep(const mlamg_gs* G, double* x, const double* b, int iterations, void* stream) {
  MLAMG_REQUIRE(G && (G->A->n_rows == 0 || (x && b)), "NULL argument");
  return gs_sweep_impl(G, x, b, iterations, nullptr, S(stream));
}

}  // extern "C"
