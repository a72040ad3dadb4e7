// CSR-stream SpMV family for gfx950 — the hot path of the V-cycle.
//
// One 256-thread workgroup per row block (<= 256 rows, <= 2048 nonzeros, built once per handle
// in runtime.cpp). Phase 1 streams the block's contiguous column-index and value ranges with
// fully coalesced loads (lane e reads nonzero e), gathers x[col] and writes the fp64 product
// into LDS. Phase 2 gives each row to one lane, which sums its products left to right from LDS
// and applies the fused epilogue. Summing in stored order with no FMA contraction
// (-ffp-contract=off) reproduces scipy sparsetools csr_matvec bit for bit:
//     sum = 0; for jj in row: sum += Ax[jj] * x[Aj[jj]]
// Epilogues cover every use of A@x in the reference V-cycle:
//   AXPBY   y = A@x (alpha=1,beta=0) or alpha*A@x + beta*y        multigrid.py:181 (P@e)
//   RESID   r = b - A@x  (+ per-block sum of r^2)                  multigrid.py:181,191
//   JACOBI  y = x + dinv_w*(b - A@x)                               MLAMG.py:145
//   JACEXP  y = x + (dinv_w*b - M@x), M = (w*Dinv)@A explicit      multigrid.py:44
//   ADD     y = y + A@x                                            multigrid.py:181 (x += P@e)
//   POLY    y = alpha*b + A@x (+ xin): one Horner step of pyamg's relaxation.polynomial, or
//           its first launch r = b - A@x with copy_to = alpha*r (+ xin)      DESIGN.md §32
// Roofline: HBM-bound. Algorithmic bytes per call = 12*nnz + 4*(n+1) + 8*n_cols + 8*n (+8n per
// extra vector the epilogue reads/writes), SURVEY.md §8(d).
// The storage formats these kernels read are built in formats.hip; formats.hpp is the seam.
#include "formats.hpp"
#include "reduce.hpp"

#include <cstdlib>

namespace mlamg {

enum EpiOp : int { EPI_AXPBY = 0, EPI_RESID = 1, EPI_JACOBI = 2, EPI_JACEXP = 3, EPI_ADD = 4,
                   EPI_FADD = 5, EPI_POLY = 6 };

struct Epi {
  double alpha, beta;
  const double* b;
  const double* xin;   // JACOBI/JACEXP: x (old iterate)
  const double* dinv;  // JACOBI/JACEXP
  double* y;           // output
  double* copy_to;     // RESID: optional x copy-back (copy_to[i] = x[i]) — used by the V-cycle
  const double* copy_from;
  double* partial;     // RESID: per-block sum of r^2 (nullable)
  const int32_t* done; // nullable: device flag; nonzero -> kernel is a no-op
  int cached;          // set by launch(): 1 = cached loads of the nonzero stream (see kCachedNnz)
  // FADD (factored SA prolongation, k_rowpat_uni only): the kernel's x operand is the virtual
  // vector t = Agg e (t_i = e[agg[i]], 0 where agg[i] < 0) and y += t - dinv * (A t)
  const int32_t* agg;
  // POLY (polynomial smoother, poly.hip). A Horner step: y = alpha * b + A x, with xin set
  // y = xin + (alpha * b + A x) (the sweep's last step; beta != 0 stands for an all-zero xin that
  // is not read). With copy_to set it is the sweep's first launch instead: y = r = b - A x (y
  // nullable) and copy_to = alpha * r, with xin set copy_to = xin + alpha * r (a one-coefficient
  // sweep; copy_to must not be the operand x). b NULL: a zero vector, as in RESID.
};

// A level operator (square) of at most kCachedNnz entries (~100 MB in CSR) is read with ordinary
// (cached) loads, so its stream stays in the 256 MB MALL from its pre-smoothing to its
// post-smoothing pass (C4 level-3 A: second pass 28 -> 22 us). Everything else — larger streams,
// and P / R, read once per cycle — uses non-temporal loads, which leave the MALL to the vectors
// the next kernel reads (cached P_2 / P_3 / R_3 streams measured 1-3 us slower each).
#ifndef MLAMG_CACHED_NNZ  // build-time A/B knob
#define MLAMG_CACHED_NNZ (8 << 20)
#endif
constexpr int64_t kCachedNnz = MLAMG_CACHED_NNZ;


// The per-row operands an epilogue reads, fetched apart from the store so kernels can issue
// these loads at the start (before the nonzero stream) and keep their latency off the tail.
struct EpiIn {
  double a = 0.0, b = 0.0, c = 0.0;
};

template <int OP>
__device__ __forceinline__ EpiIn epi_load(int row, const Epi& e) {
  EpiIn v;
  if constexpr (OP == EPI_AXPBY) {
    if (e.beta != 0.0) v.a = e.y[row];
    if (e.copy_to) v.c = e.dinv[row];
  } else if constexpr (OP == EPI_RESID) {
    v.a = e.b ? e.b[row] : 0.0;  // b NULL: a zero right-hand side (+0.0: the same bits)
    if (e.copy_to) {
      v.b = e.copy_from[row];
      if (e.dinv) v.c = e.dinv[row];
    }
  } else if constexpr (OP == EPI_JACOBI || OP == EPI_JACEXP) {
    v.a = e.b ? e.b[row] : 0.0;
    v.b = e.xin[row];
    v.c = e.dinv[row];
  } else if constexpr (OP == EPI_FADD) {
    v.a = e.y[row];
    v.c = e.dinv[row];
  } else if constexpr (OP == EPI_POLY) {
    v.a = e.b ? e.b[row] : 0.0;
    if (e.xin) v.b = e.xin[row];  // else +0.0
  } else {  // EPI_ADD
    v.a = e.y[row];
  }
  return v;
}

template <int OP>
__device__ __forceinline__ double epi_store(int row, double s, const EpiIn& v, const Epi& e) {
  if constexpr (OP == EPI_AXPBY) {
    double y;
    if (e.beta == 0.0) {
      y = (e.alpha == 1.0) ? s : e.alpha * s;
    } else {
      y = e.alpha * s + e.beta * v.a;
    }
    e.y[row] = y;
    // restriction fused with the next level's zero-guess sweep: x = Dinv_w * b (0 + d*(b - 0))
    if (e.copy_to) e.copy_to[row] = v.c * y;
    return 0.0;
  } else if constexpr (OP == EPI_RESID) {
    const double r = v.a - s;
    if (e.y) e.y[row] = r;  // NULL: r is only needed for the norm and the fused sweep
    // optional copy-back of the iterate; with dinv also the next cycle's first Jacobi sweep
    // x + dinv*r, fused here (same two roundings as the stand-alone sweep)
    if (e.copy_to) e.copy_to[row] = e.dinv ? v.b + v.c * r : v.b;
    return r * r;
  } else if constexpr (OP == EPI_JACOBI) {
    const double r = v.a - s;
    e.y[row] = v.b + v.c * r;
    return 0.0;
  } else if constexpr (OP == EPI_JACEXP) {
    const double t1 = v.c * v.a;
    e.y[row] = v.b + (t1 - s);
    return 0.0;
  } else if constexpr (OP == EPI_FADD) {
    e.y[row] = v.a + (v.b - v.c * s);
    return 0.0;
  } else if constexpr (OP == EPI_POLY) {
    if (e.copy_to) {  // first launch of a sweep: r and h_0 = c_0 r (one coefficient: x + c_0 r)
      const double r = v.a - s;
      if (e.y) e.y[row] = r;
      const double h = e.alpha * r;
      e.copy_to[row] = e.xin ? v.b + h : h;
    } else {  // h = c_i r + A h, the last one added to x (each operation rounds on its own)
      const double t = e.alpha * v.a;
      const double h = t + s;
      e.y[row] = (e.xin || e.beta != 0.0) ? v.b + h : h;
    }
    return 0.0;
  } else {  // EPI_ADD
    e.y[row] = v.a + s;
    return 0.0;
  }
}

template <int OP>
__device__ __forceinline__ double epilogue(int row, double s, const Epi& e) {
  return epi_store<OP>(row, s, epi_load<OP>(row, e), e);
}

// XCD-aware block order: the dispatcher deals blocks round-robin over the 8 XCDs (b % 8 share
// one L2), so logical block = contiguous chunk per XCD. Neighbouring row blocks then share x
// lines in the same L2 (7-point stencil: rows i +- 1, +- n, +- n^2). Bijective for any nb.
__device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t nb) {
  const int64_t q = nb >> 3, r = nb & 7, g = b & 7, i = b >> 3;
  return (g < r ? g * (q + 1) : r * (q + 1) + (g - r) * q) + i;
}

template <int OP, bool NORM>
__global__ __launch_bounds__(kThreads) void k_csr_stream(const int32_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const double* __restrict__ vals,
                                                         const int32_t* __restrict__ blk,
                                                         const double* __restrict__ x, Epi ep) {
  __shared__ double prod[kBlockNnz];
  __shared__ int32_t rp[kBlockRows + 1];
  __shared__ double red[kThreads / 64];
  if (ep.done && *ep.done) return;
  const int b = (int)xcd_block(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  const int r0 = blk[b];
  const int r1 = blk[b + 1];
  const int nr = r1 - r0;
  const int e0 = indptr[r0];
  const int ne = indptr[r1] - e0;
  double sq = 0.0;
  if (ne <= kBlockNnz) {
    static_assert(kBlockRows <= kThreads, "one row per thread in phase 2");
    EpiIn pre;
    if (tid < nr) pre = epi_load<OP>(r0 + tid, ep);
    // row pointers to registers now, to LDS after the gathers (an LDS store waits for its load,
    // which would hold back the entry loads behind it)
    const int rpa = indptr[r0 + min(tid, nr)];
    const int rpb = tid == 0 ? indptr[r1] : 0;  // t = kThreads when nr == kBlockRows == kThreads
    const int32_t* ci = indices + e0;
    const double* cv = vals + e0;
    // all kBlockNnz/kThreads loads of a lane issued back to back: the x gathers depend on the
    // index loads, so without the unroll each iteration pays two full memory round trips
    constexpr int U = kBlockNnz / kThreads;
    int32_t cc[U];
    double vv[U], xv[U];
    if (ep.cached) {  // uniform: one unrolled load sequence or the other
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = tid + u * kThreads;
        cc[u] = e < ne ? ci[e] : -1;
        vv[u] = e < ne ? cv[e] : 0.0;
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = tid + u * kThreads;
        cc[u] = e < ne ? __builtin_nontemporal_load(ci + e) : -1;
        vv[u] = e < ne ? __builtin_nontemporal_load(cv + e) : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xv[u] = cc[u] >= 0 ? x[cc[u]] : 0.0;
    if (tid <= nr) rp[tid] = rpa - e0;
    if (tid == 0 && nr == kThreads) rp[kThreads] = rpb - e0;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tid + u * kThreads < ne) prod[tid + u * kThreads] = vv[u] * xv[u];
    __syncthreads();
    if (tid < nr) {
      const int t = tid;
      double s = 0.0;
      const int ka = rp[t], kb = rp[t + 1];
      int k = ka;
      for (; k + 4 <= kb; k += 4) {
        const double p0 = prod[k], p1 = prod[k + 1], p2 = prod[k + 2], p3 = prod[k + 3];
        s += p0;
        s += p1;
        s += p2;
        s += p3;
      }
      for (; k < kb; ++k) s += prod[k];
      sq += epi_store<OP>(r0 + t, s, pre, ep);
    }
  } else {
    // one over-long row: stream it through LDS in chunks, lane 0 keeps the ordered sum
    double s = 0.0;
    for (int c = 0; c < ne; c += kBlockNnz) {
      const int m = min(kBlockNnz, ne - c);
      for (int e = tid; e < m; e += kThreads) prod[e] = vals[e0 + c + e] * x[indices[e0 + c + e]];
      __syncthreads();
      if (tid == 0)
        for (int k = 0; k < m; ++k) s += prod[k];
      __syncthreads();
    }
    if (tid == 0) sq += epilogue<OP>(r0, s, ep);
  }
  if constexpr (NORM) {
    // fixed-order block reduction -> deterministic partials
    const double t = block_sum<kThreads>(sq, red);
    if (tid == 0) ep.partial[b] = t;
  }
}

// Sum `n` partials in a fixed order with one workgroup, write sqrt to out (device scalar),
// optionally also to hist[*counter] and raise done flag when <= tol.
__global__ __launch_bounds__(1024) void k_finalize_norm(const double* __restrict__ partial, int n,
                                                        double* out, double* hist,
                                                        int32_t* counter, int32_t* done,
                                                        double tol) {
  __shared__ double red[16];
  if (done && *done) return;
  const double t = partials_total<1024>(partial, n, red);
  if (threadIdx.x == 0) {
    const double nrm = sqrt(t);
    if (out) *out = nrm;
    const int c = counter ? *counter : 0;
    if (hist) hist[c] = nrm;
    if (counter) *counter = c + 1;
    if (done && tol >= 0.0 && nrm <= tol) *done = 1;
  }
}

// ---------------------------------------------------------------- SELL-64 variant
// One wave per slice of 64 consecutive rows, one lane per row; entry k of the slice's rows is
// stored contiguously for the 64 lanes (col-major), so every load instruction of the wave reads
// 256 B of indices / 512 B of values with no LDS round trip and no row pointers. Lane i sums
// its row in stored order, skipping the col = -1 padding: the same bits as csr_matvec.
template <int OP, bool NORM>
__global__ __launch_bounds__(kThreads) void k_sell(const int64_t* __restrict__ sp,
                                                   const int32_t* __restrict__ cols,
                                                   const double* __restrict__ vals,
                                                   const int32_t* __restrict__ perm,
                                                   int64_t n_rows, int64_t n_slices,
                                                   const double* __restrict__ x, Epi ep) {
  __shared__ double red[kThreads / 64];
  if (ep.done && *ep.done) return;
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t slice = lb * (kThreads / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  double sq = 0.0;
  if (slice < n_slices) {
    const int64_t srow = slice * 64 + lane;
    const int prow = srow < n_rows ? (perm ? perm[srow] : (int)srow) : 0;
    EpiIn pre;
    if (srow < n_rows) pre = epi_load<OP>(prow, ep);
    const int64_t base = sp[slice];
    const int w = (int)((sp[slice + 1] - base) >> 6);
    const int32_t* c = cols + base + lane;
    const double* v = vals + base + lane;
    double s = 0.0;
    // batches of 8 with predicated tails, so a 7-point row issues all its loads at once
    for (int k = 0; k < w; k += 8) {
      int32_t cc[8];
      double vv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        cc[u] = k + u < w ? __builtin_nontemporal_load(c + (int64_t)(k + u) * 64) : -1;
        vv[u] = k + u < w ? __builtin_nontemporal_load(v + (int64_t)(k + u) * 64) : 0.0;
      }
      double xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) xv[u] = cc[u] >= 0 ? x[cc[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (cc[u] >= 0) s += vv[u] * xv[u];
    }
    if (srow < n_rows) sq = epi_store<OP>(prow, s, pre, ep);
  }
  if constexpr (NORM) {
    const double t = block_sum<kThreads>(sq, red);
    if (threadIdx.x == 0) ep.partial[lb] = t;
  }
}

// ---------------------------------------------------------------- dictionary-coded SELL-64
// k_sell with 2-byte elements: code = offset index | value index << 8 into per-matrix tables
// (staged in LDS), col = row + offset. For a constant-coefficient stencil (C4: 7 offsets, 2
// values) the matrix stream drops from 12 to 2 bytes per nonzero; the products, and the order
// they are summed in, are exactly SELL's, hence scipy's.
template <int OP, bool NORM, int SPW>
__global__ __launch_bounds__(kThreads) void k_sell_dict(const int64_t* __restrict__ dp,
                                                        const uint16_t* __restrict__ codes,
                                                        const int32_t* __restrict__ dict_off,
                                                        const double* __restrict__ dict_val,
                                                        const int32_t* __restrict__ perm,
                                                        int64_t n_rows, int64_t n_slices,
                                                        const double* __restrict__ x, Epi ep) {
  // SPW slices per wave (lane j holds row j of each): their loads are issued together, so a
  // wave keeps SPW x 7 gathers in flight on a 7-point stencil; each lane fetches its next 8
  // codes with one 16-byte load
  __shared__ int32_t offt[256];
  __shared__ double valt[256];
  __shared__ double red[kThreads / 64];
  if (ep.done && *ep.done) return;
  static_assert(kThreads == 256, "one table entry per thread");
  offt[threadIdx.x] = dict_off[threadIdx.x];
  valt[threadIdx.x] = dict_val[threadIdx.x];
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t slice0 = (lb * (kThreads / 64) + (threadIdx.x >> 6)) * SPW;
  const int lane = threadIdx.x & 63;
  int row[SPW], ng[SPW];
  int64_t srow[SPW], base[SPW];
  EpiIn pre[SPW];
  int gmax = 0;
#pragma unroll
  for (int q = 0; q < SPW; ++q) {
    const int64_t sl = slice0 + q;
    srow[q] = sl * 64 + lane;
    row[q] = srow[q] < n_rows ? (perm ? perm[srow[q]] : (int)srow[q]) : 0;
    if (srow[q] < n_rows) pre[q] = epi_load<OP>(row[q], ep);
    base[q] = sl < n_slices ? dp[sl] : 0;
    ng[q] = sl < n_slices ? (int)((dp[sl + 1] - base[q]) >> 9) : 0;  // groups of 8 x 64 codes
    gmax = ng[q] > gmax ? ng[q] : gmax;
  }
  __syncthreads();
  double acc[SPW];
#pragma unroll
  for (int q = 0; q < SPW; ++q) acc[q] = 0.0;
  for (int g = 0; g < gmax; ++g) {
    uint16_t cc[SPW][8];
#pragma unroll
    for (int q = 0; q < SPW; ++q) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      u32x4 v = {0x00FF00FFu, 0x00FF00FFu, 0x00FF00FFu, 0x00FF00FFu};
      if (g < ng[q])
        v = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4*>(codes + base[q] + ((int64_t)g << 9)) + lane);
      const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        cc[q][2 * u] = (uint16_t)(wv[u] & 0xFFFFu);
        cc[q][2 * u + 1] = (uint16_t)(wv[u] >> 16);
      }
    }
    double xv[SPW][8];
#pragma unroll
    for (int q = 0; q < SPW; ++q)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        xv[q][u] = (cc[q][u] & 0xFF) != 0xFF ? x[row[q] + offt[cc[q][u] & 0xFF]] : 0.0;
#pragma unroll
    for (int q = 0; q < SPW; ++q)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if ((cc[q][u] & 0xFF) != 0xFF) acc[q] += valt[cc[q][u] >> 8] * xv[q][u];
  }
  double sq = 0.0;
#pragma unroll
  for (int q = 0; q < SPW; ++q)
    if (srow[q] < n_rows) sq += epi_store<OP>(row[q], acc[q], pre[q], ep);
  if constexpr (NORM) {
    const double t = block_sum<kThreads>(sq, red);
    if (threadIdx.x == 0) ep.partial[lb] = t;
  }
}

// ---------------------------------------------------------------- row-pair pattern format
// A constant-coefficient stencil has few distinct rows: as sequences of (col - row, value)
// pairs in stored order, C4's Laplacian has 27 (interior / face / edge / corner rows). This
// format keys rows two at a time: pair (2i, 2i+1) carries a one-byte id into <= 255 pair
// patterns held in LDS, each the merge of its two rows' entries by column offset, with flags
// saying which row an entry belongs to. Lane per pair: an offset both rows have is ONE 16-byte
// load x[2i+off .. 2i+off+1], and the epilogue vectors move as 16-byte pairs, so the matrix
// stream is half a byte per row and a wave instruction moves 1 KB (a lane per row leaves the
// kernel latency-bound at ~3.3 TB/s). Each row still sums its own entries in stored (ascending
// column) order: the products and their order are CSR's, hence scipy's bits.

typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef double dbl2u __attribute__((ext_vector_type(2), aligned(8)));  // 8-byte aligned pair

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// v0 = p[i], v1 = p[i+1] (i even; p[i+1] only when both): one 16-byte load when p is aligned
__device__ __forceinline__ void ld2(const double* p, int i, bool both, double& v0, double& v1) {
  if (both && al16(p)) {
    const dbl2 t = *reinterpret_cast<const dbl2*>(p + i);
    v0 = t.x;
    v1 = t.y;
  } else {
    v0 = p[i];
    v1 = both ? p[i + 1] : 0.0;
  }
}

#ifndef MLAMG_ST_NT
#define MLAMG_ST_NT 0
#endif
__device__ __forceinline__ void st2(double* p, int i, bool both, double v0, double v1) {
  if (both && al16(p)) {
    dbl2 t;
    t.x = v0;
    t.y = v1;
    if constexpr (MLAMG_ST_NT)
      __builtin_nontemporal_store(t, reinterpret_cast<dbl2*>(p + i));
    else
      *reinterpret_cast<dbl2*>(p + i) = t;
  } else {
    p[i] = v0;
    if (both) p[i + 1] = v1;
  }
}

// epi_load for rows r, r+1
// (no_dinv: the dinv operand comes from the caller's pattern table instead of memory)
// (no_x: the x operand — JACOBI's xin, RESID's copy_from — equals the SpMV's x and comes from
// the caller's LDS window instead of memory)
template <int OP>
__device__ __forceinline__ void epi_load2(int r, bool both, const Epi& e, EpiIn& u, EpiIn& w,
                                          bool no_dinv, bool no_x = false) {
  if constexpr (OP == EPI_AXPBY) {
    if (e.beta != 0.0) ld2(e.y, r, both, u.a, w.a);
    if (e.copy_to && !no_dinv) ld2(e.dinv, r, both, u.c, w.c);
  } else if constexpr (OP == EPI_RESID) {
    if (e.b) ld2(e.b, r, both, u.a, w.a);  // b NULL: zero right-hand side (u.a = w.a = +0.0)
    if (e.copy_to) {
      if (!no_x) ld2(e.copy_from, r, both, u.b, w.b);
      if (e.dinv && !no_dinv) ld2(e.dinv, r, both, u.c, w.c);
    }
  } else if constexpr (OP == EPI_JACOBI || OP == EPI_JACEXP) {
    if (e.b) ld2(e.b, r, both, u.a, w.a);
    if (!no_x) ld2(e.xin, r, both, u.b, w.b);
    if (!no_dinv) ld2(e.dinv, r, both, u.c, w.c);
  } else if constexpr (OP == EPI_FADD) {
    ld2(e.y, r, both, u.a, w.a);
    if (!no_dinv) ld2(e.dinv, r, both, u.c, w.c);  // t (u.b, w.b) comes from the x window
  } else if constexpr (OP == EPI_POLY) {
    if (e.b) ld2(e.b, r, both, u.a, w.a);
    if (e.xin) ld2(e.xin, r, both, u.b, w.b);
  } else {  // EPI_ADD
    ld2(e.y, r, both, u.a, w.a);
  }
}

// epi_store's arithmetic for one row, returned instead of stored: the output, the copy_to value
// (AXPBY/RESID) and the row's r^2 (RESID)
template <int OP>
__device__ __forceinline__ double epi_value(double s, const EpiIn& v, const Epi& e, double& c,
                                            double& sq) {
  if constexpr (OP == EPI_AXPBY) {
    const double y = (e.beta == 0.0) ? ((e.alpha == 1.0) ? s : e.alpha * s)
                                     : e.alpha * s + e.beta * v.a;
    c = v.c * y;
    return y;
  } else if constexpr (OP == EPI_RESID) {
    const double r = v.a - s;
    c = e.dinv ? v.b + v.c * r : v.b;
    sq = r * r;
    return r;
  } else if constexpr (OP == EPI_JACOBI) {
    const double r = v.a - s;
    return v.b + v.c * r;
  } else if constexpr (OP == EPI_JACEXP) {
    const double t1 = v.c * v.a;
    return v.b + (t1 - s);
  } else if constexpr (OP == EPI_FADD) {
    return v.a + (v.b - v.c * s);  // x + (t - (w / a_ii) (A t)): x + P e, P = (I - w D^-1 A) Agg
  } else if constexpr (OP == EPI_POLY) {
    if (e.copy_to) {
      const double r = v.a - s;
      const double h = e.alpha * r;
      c = e.xin ? v.b + h : h;
      return r;
    }
    const double t = e.alpha * v.a;
    const double h = t + s;
    return (e.xin || e.beta != 0.0) ? v.b + h : h;
  } else {  // EPI_ADD
    return v.a + s;
  }
}

template <int OP>
__device__ __forceinline__ double epi_store2(int r, bool both, double s0, double s1,
                                             const EpiIn& u, const EpiIn& w, const Epi& e) {
  double c0 = 0.0, c1 = 0.0, q0 = 0.0, q1 = 0.0;
  const double y0 = epi_value<OP>(s0, u, e, c0, q0);
  const double y1 = epi_value<OP>(s1, w, e, c1, q1);
  if ((OP != EPI_RESID && OP != EPI_POLY) || e.y) st2(e.y, r, both, y0, y1);
  if constexpr (OP == EPI_AXPBY || OP == EPI_RESID || OP == EPI_POLY)
    if (e.copy_to) st2(e.copy_to, r, both, c0, c1);
  return both ? q0 + q1 : q0;
}

// One pair's row sums (rows r, r+1; patterns padded to multiples of 8 entries from a) from the
// LDS tables: vv[e] = (row 2i's value, row 2i+1's value), of[e] = (column offset, row 2i mask,
// row 2i+1 mask, flags).
template <int K>
__device__ __forceinline__ void rowpair_sums(const double* __restrict__ x, int64_t n_cols, int r,
                                             int a, int len, const dbl2* vv, const int4* of,
                                             double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
  if (len > 0 && (of[a].w & 4)) {
    // "wide" pattern: x[2i+off .. 2i+off+1] is in range for every entry, so each entry is one
    // 16-byte buffer load; an entry a row does not have is masked to +0.0 (its table value is
    // 0.0 too), and adding +0.0 leaves the sum's bits alone (a sum that starts at +0.0 is never
    // -0.0), so the products and the order each row sums them in are CSR's
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(n_cols * 8), 0x00020000);
    const int r8 = r * 8;
    for (int k = 0; k < len; k += K) {
      u32x4 t[K];
      int4 f[K];
#pragma unroll
      for (int q = 0; q < K; ++q) {
        f[q] = of[a + k + q];
        t[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, r8 + f[q].x * 8, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < K; ++q) {
        const dbl2 v = vv[a + k + q];
        const uint64_t b0 = ((uint64_t)(t[q].y & (uint32_t)f[q].y) << 32) | (t[q].x & (uint32_t)f[q].y);
        const uint64_t b1 = ((uint64_t)(t[q].w & (uint32_t)f[q].z) << 32) | (t[q].z & (uint32_t)f[q].z);
        s0 += v.x * __longlong_as_double((long long)b0);
        s1 += v.y * __longlong_as_double((long long)b1);
      }
    }
    return;
  }
  // edge pairs (first / last rows of the matrix, odd tail): per-row loads as needed
  const double* xr = x + r;
  for (int k = 0; k < len; k += K) {
    double x0[K], x1[K];
    int fl[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const int4 f = of[a + k + q];
      fl[q] = f.w;
      x0[q] = (fl[q] & 1) ? xr[f.x] : 0.0;
      x1[q] = (fl[q] & 2) ? xr[f.x + 1] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
      if (fl[q] & 1) s0 += vv[a + k + q].x * x0[q];
      if (fl[q] & 2) s1 += vv[a + k + q].y * x1[q];
    }
  }
}

// CH chunks of 256 pairs per workgroup (tables staged once; the next chunk's pattern ids are
// fetched while the current chunk gathers). MLAMG_RP_WAVES: minimum waves per SIMD the register
// allocation must leave room for (0 = compiler's choice; build-time knob for A/B runs)
// 5 (round 3): the end-of-cycle instantiation (residual + norm + fused next sweep) took 115
// VGPRs, 4 waves per SIMD; at 5 it fits 96 with no spill (the others 91-94): that kernel 67 -> 58
// us, the cycle 813 -> 802 us traced, bench +0.6-1.2 % alternating on one box (6: spills, 10 %
// slower; profiles/r03/final/ab_rowpair_waves*.txt)
#ifndef MLAMG_RP_WAVES
#define MLAMG_RP_WAVES 5
#endif
template <int OP, bool NORM, int CH, int K>
__global__ __launch_bounds__(kThreads)
__attribute__((amdgpu_waves_per_eu(MLAMG_RP_WAVES > 0 ? MLAMG_RP_WAVES : 1, 8)))
void k_rowpair(const uint8_t* __restrict__ pid,
                                                      const int32_t* __restrict__ pat_ptr,
                                                      const int4* __restrict__ pat_of,
                                                      const dbl2* __restrict__ pat_vv,
                                                      int n_ent, int64_t n_rows, int64_t n_cols,
                                                      const double* __restrict__ dinv_att,
                                                      const dbl2* __restrict__ pat_dinv,
                                                      int n_pat, const double* __restrict__ x,
                                                      Epi ep) {
  // LDS: vv[n_ent] (16 B) | of[n_ent] (16 B) | dinv[n_pat] (16 B) | starts[257]
  extern __shared__ dbl2 rp_lds[];
  __shared__ double red[kThreads / 64];
  if (ep.done && *ep.done) return;
  dbl2* vv = rp_lds;
  int4* of = reinterpret_cast<int4*>(rp_lds + n_ent);
  dbl2* dt = reinterpret_cast<dbl2*>(of + n_ent);
  int32_t* pst = reinterpret_cast<int32_t*>(dt + n_pat);
  // the epilogue's dinv is the vector attached to this operator (mlamg_csr_attach_dinv): its
  // entries are per-pattern constants, verified at attach time, read from LDS
  const bool tab_dinv = ep.dinv != nullptr && ep.dinv == dinv_att;
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t pr0 = lb * CH * kThreads + threadIdx.x;  // this lane's pair in chunk 0
  int p = 2 * pr0 < n_rows ? (int)pid[pr0] : 0;
  for (int i = threadIdx.x; i < n_ent; i += kThreads) {
    vv[i] = pat_vv[i];
    of[i] = pat_of[i];
  }
  for (int i = threadIdx.x; i < 257; i += kThreads) pst[i] = pat_ptr[i];
  if (tab_dinv)
    for (int i = threadIdx.x; i < n_pat; i += kThreads) dt[i] = pat_dinv[i];
  double sq = 0.0;
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < CH; ++c) {
    const int64_t pr = pr0 + (int64_t)c * kThreads;
    const bool ok0 = 2 * pr < n_rows;
    const bool both = 2 * pr + 1 < n_rows;
    const int r = ok0 ? (int)(2 * pr) : 0;
    const int p_next =
        (c + 1 < CH && 2 * (pr + kThreads) < n_rows) ? (int)pid[pr + kThreads] : 0;
    EpiIn u, w;
    if (ok0) epi_load2<OP>(r, both, ep, u, w, tab_dinv);
    if (tab_dinv) {
      const dbl2 d = dt[p];
      u.c = d.x;
      w.c = d.y;
    }
    const int a = pst[p];
    const int len = ok0 ? pst[p + 1] - a : 0;
    double s0, s1;
    rowpair_sums<K>(x, n_cols, r, a, len, vv, of, s0, s1);
    if (ok0) sq += epi_store2<OP>(r, both, s0, s1, u, w, ep);
    p = p_next;
  }
  if constexpr (NORM) {
    const double t = block_sum<kThreads>(sq, red);
    if (threadIdx.x == 0) ep.partial[lb] = t;
  }
}

// ---------------------------------------------------------------- uniform row-pair stencils
// k_rowpat_uni: the row-pair pattern format for operators whose pattern entries all come from
// ONE list of <= 8 column offsets with one value per (offset, row parity) — constant-coefficient
// stencils, where the patterns only differ in which neighbours a boundary row lacks (C4 A_0: 27
// patterns over the 7 offsets -n^2 -n -1 0 1 n n^2). A pattern is then a 16-bit mask (the slots
// row 2i and row 2i+1 have) in a 512-byte LDS table and the values are kernel arguments. Same pid
// bytes as k_rowpair; chunk c of workgroup lb holds pairs lb*CH*256 + c*256 + lane (CH = 2 by
// default; with CH = kRpChunks the norm partials are k_rowpair's too), and every product and
// sum is k_rowpair's, i.e. scipy's (an entry a row lacks is a +0.0 operand: a sum started at
// +0.0 is never -0.0, so adding it changes no bit). The x operands within +-halo rows come from an LDS
// window of the workgroup's 2 CH 256 rows plus the halo, staged once with 16-byte loads
// (k_rowpair issues 7 16-byte texture loads per pair; tools/stencil_lab.hip k_pair_tile: 24.4 us
// for the C4 stencil against 32.6 us with every neighbour a global load): even offsets are one
// aligned 16-byte LDS read, -1 / +1 take the neighbouring pairs' reads. The far offsets (C4:
// +-n^2) are 16-byte global loads, all issued before the staging. An epilogue operand equal to
// x (Jacobi's xin, the fused sweep's copy_from) comes from the window. Every load is
// branch-free: an address is clamped into x and the lanes it does not cover are selected to
// zero (a branch join makes the compiler wait for every load in flight).
// LY: slot layout (kinds in slot order; 0 even window offset, 1 offset -1, 2 offset +1, 3 far):
// 1 = {3,0,1,0,2,0,3} (3-D 7-point), 2 = {0,1,0,2,0} (2-D 5-point, +-n staged),
// 3 = {3,1,0,2,3} (2-D 5-point, +-n far), 4 = layout 1 with alternate far offsets (a
// row-partitioned slab's ghost planes, RpUni::alt_*), 0 = any (run-time kinds, alternates too).
// Only layouts 0 and 4 compare pair indices against the alternate ranges.
__device__ __forceinline__ dbl2 x16(const double* __restrict__ x, int64_t g, int64_t n) {
  const int64_t gc = g < 0 ? 0 : (g > n - 2 ? n - 2 : g);
  const dbl2 t = *reinterpret_cast<const dbl2u*>(x + gc);
  // g == gc: both in range; g == -1: (0, x[0]) = (0, t.x); g == n - 1: (x[n-1], 0) = (t.y, 0)
  dbl2 o;
  o.x = g == gc ? t.x : (g == n - 1 ? t.y : 0.0);
  o.y = g == gc ? t.y : (g == -1 ? t.x : 0.0);
  return o;
}

// x16 for the virtual operand t = Agg e of the factored prolongation (EPI_FADD): t_g =
// e[agg[g]] (0 where agg[g] < 0 or g outside [0, n)), branch-free like x16
__device__ __forceinline__ dbl2 t16(const int32_t* __restrict__ agg, const double* __restrict__ e,
                                    int64_t g, int64_t n) {
  const int64_t gc = g < 0 ? 0 : (g > n - 2 ? n - 2 : g);
  const int a0 = agg[gc], a1 = agg[gc + 1];
  const double v0 = e[a0 < 0 ? 0 : a0], v1 = e[a1 < 0 ? 0 : a1];
  const double t0 = a0 < 0 ? 0.0 : v0, t1 = a1 < 0 ? 0.0 : v1;
  dbl2 o;
  o.x = g == gc ? t0 : (g == n - 1 ? t1 : 0.0);
  o.y = g == gc ? t1 : (g == -1 ? t0 : 0.0);
  return o;
}
#ifndef MLAMG_UNI_BUF  // build-time A/B knob: x operands through a buffer resource with 32-bit
#define MLAMG_UNI_BUF 1  // offsets (1) or flat 64-bit addresses (0): 74 -> 62 VGPRs (6 -> 8
#endif                   // waves per SIMD), C4 A_0 cold 43.1 -> 41.9 us
// x16 through a buffer resource with 32-bit index arithmetic (n * 8 < 2^31, checked where the
// uniform form is built): no 64-bit address registers per load
__device__ __forceinline__ dbl2 x16r(__amdgpu_buffer_rsrc_t rs, int g, int n) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int gc = g < 0 ? 0 : (g > n - 2 ? n - 2 : g);
  const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, gc * 8, 0, 0);
  const double t0 = __builtin_bit_cast(double, ((uint64_t)t.y << 32) | t.x);
  const double t1 = __builtin_bit_cast(double, ((uint64_t)t.w << 32) | t.z);
  dbl2 o;
  o.x = g == gc ? t0 : (g == n - 1 ? t1 : 0.0);
  o.y = g == gc ? t1 : (g == -1 ? t0 : 0.0);
  return o;
}
template <int OP>
__device__ __forceinline__ dbl2 uni_x16(const double* __restrict__ x, int64_t g, int64_t n,
                                        const Epi& ep, __amdgpu_buffer_rsrc_t rs) {
  if constexpr (OP == EPI_FADD)
    return t16(ep.agg, x, g, n);
  else if constexpr (MLAMG_UNI_BUF)
    return x16r(rs, (int)g, (int)n);
  else
    return x16(x, g, n);
}

template <int LY>
__device__ __forceinline__ int uni_kind(const RpUni& U, int q) {
  constexpr int k1[7] = {3, 0, 1, 0, 2, 0, 3}, k2[5] = {0, 1, 0, 2, 0}, k3[5] = {3, 1, 0, 2, 3};
  if constexpr (LY == 1) return k1[q < 7 ? q : 0];
  if constexpr (LY == 2) return k2[q < 5 ? q : 0];
  if constexpr (LY == 3) return k3[q < 5 ? q : 0];
  if constexpr (LY == 4) return k1[q < 7 ? q : 0];
  return U.kind[q];
}
template <int LY>
__device__ __forceinline__ int uni_k(const RpUni& U) {
  return LY == 1 || LY == 4 ? 7 : (LY == 2 || LY == 3) ? 5 : U.k;
}

#ifndef MLAMG_UNI_DBG
#define MLAMG_UNI_DBG 0  // timing-only builds (tools/build_variant.sh): 1 no masks, 2 no id
#endif                   // loads, 4 no far loads, 8 no stores — results are then wrong
#ifndef MLAMG_UNI_EPF  // build-time A/B knob: epilogue operands prefetched one chunk ahead
#define MLAMG_UNI_EPF 2  // 0 never, 1 always, 2 in the NORM form (the end-of-cycle pass: traced
#endif                   // 66.7 -> 58.6 us; the other passes got slower: 51.8 -> 55.3 us)
#ifndef MLAMG_UNI_WPE  // build-time A/B knob: minimum waves per SIMD for k_rowpat_uni (0: free)
#define MLAMG_UNI_WPE 0
#endif
#ifndef MLAMG_UNI_PFA  // build-time A/B knob: with CH <= 2 chunks, every chunk's id and far
#define MLAMG_UNI_PFA 1  // operands issued before the window staging (1), not one chunk ahead (0):
#endif                   // C4 A_0 cold 45.0 -> 43.0 us, resid+norm 64 -> 52 us
template <int OP, bool NORM, int CH, int LY>
__global__ __launch_bounds__(kThreads)
__attribute__((amdgpu_waves_per_eu(MLAMG_UNI_WPE > 0 ? MLAMG_UNI_WPE : 1, 8)))
void k_rowpat_uni(
    const uint8_t* __restrict__ pid, const uint16_t* __restrict__ pat_msk, int n_pat,
    int64_t n_rows, int64_t n_cols, const double* __restrict__ dinv_att,
    const dbl2* __restrict__ pat_dinv, RpUni U, const double* __restrict__ x, Epi ep) {
  // LDS: window[CH 256 + halo] (dbl2) | dinv[n_pat] (dbl2) | mask[256] (uint16)
  extern __shared__ dbl2 uni_lds[];
  __shared__ double red[kThreads / 64];
  if (ep.done && *ep.done) return;
  const int hw = U.halo >> 1;  // halo in pairs
  const int nwin = CH * kThreads + 2 * hw;
  dbl2* win = uni_lds;
  dbl2* dt = win + nwin;
  uint16_t* msk = reinterpret_cast<uint16_t*>(dt + n_pat);
  const bool tab_dinv = ep.dinv != nullptr && ep.dinv == dinv_att;
  bool x_op = false;
  if constexpr (OP == EPI_JACOBI || OP == EPI_JACEXP) x_op = ep.xin == x;
  if constexpr (OP == EPI_RESID) x_op = ep.copy_to != nullptr && ep.copy_from == x;
  if constexpr (OP == EPI_FADD) x_op = true;  // t_i, t_i+1: the window's own pair
  const int K = uni_k<LY>(U);
  const __amdgpu_buffer_rsrc_t rsx =
      __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(n_cols * 8), 0x00020000);
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t p0 = lb * CH * kThreads;  // the workgroup's first pair
  const int64_t T0 = 2 * p0 - U.halo;     // its first window row (even)
  const int64_t pa = p0 + threadIdx.x;
  // far offsets (slot order), as two scalars: an array here ends up in scratch memory once a
  // select picks between its element and an alternate offset (the select becomes one of
  // addresses; 8-12 B per lane, the C4 A_0 pass 45 -> 57 us cold)
  int fo0 = 0, fo1 = 0;
  {
    int nf = 0;
#pragma unroll
    for (int q = 0; q < kRpUniMax; ++q)
      if (q < K && uni_kind<LY>(U, q) == 3) {
        if (nf == 0) fo0 = U.off[q];
        if (nf == 1) fo1 = U.off[q];
        ++nf;
      }
  }
  static_assert(kRpUniFar == 2, "far slots: fo0, fo1");
  constexpr int NF = LY == 1 || LY == 3 || LY == 4 ? 2 : (LY == 2 ? 0 : kRpUniFar);
  constexpr int NFR = NF > 0 ? NF : 1;
  constexpr bool ALT = LY == 0 || LY == 4;
  // far slot t's offset for pair p (an alternate one on the pairs [alt_lo, alt_hi))
#define MLAMG_FAR_OFF(t, p)                                                          \
  ((ALT && (p) >= U.alt_lo[t] && (p) < U.alt_hi[t]) ? U.alt_off[t] : ((t) == 0 ? fo0 : fo1))
  // chunk 0's id and far operands, then the window: all loads before the first LDS store
  constexpr bool PFA = MLAMG_UNI_PFA != 0;
  constexpr int CHA = PFA && CH <= 2 ? CH : 1;  // chunks whose id and far operands go out first
  int pall[CHA];
  dbl2 fall[CHA][NFR];
#pragma unroll
  for (int c = 0; c < CHA; ++c) {
    const int64_t pc = pa + (int64_t)c * kThreads;
    pall[c] = (MLAMG_UNI_DBG & 2) ? 13 : pid[2 * pc < n_rows ? pc : 0];
#pragma unroll
    for (int t = 0; t < NF; ++t)
      fall[c][t] = (MLAMG_UNI_DBG & 4) ? dbl2{0.0, 0.0}
                                        : uni_x16<OP>(x, 2 * pc + MLAMG_FAR_OFF(t, pc), n_cols, ep, rsx);
  }
  int pcur = pall[0];
  dbl2 fcur[NFR];
#pragma unroll
  for (int t = 0; t < NF; ++t) fcur[t] = fall[0][t];
  // EPF: the epilogue's row operands (b, ...) of chunk 0 go out here too, and chunk c + 1's
  // with its id and far operands, so no chunk waits for its own epilogue loads
  constexpr bool EPF = MLAMG_UNI_EPF == 1 || (MLAMG_UNI_EPF == 2 && NORM);
  EpiIn unx, wnx;
  if constexpr (EPF) {
    if (2 * pa < n_rows) epi_load2<OP>((int)(2 * pa), 2 * pa + 1 < n_rows, ep, unx, wnx, tab_dinv, x_op);
  }
  constexpr int WQ = CH + 2;  // window slots per thread (halo <= 256 pairs a side)
  dbl2 wv[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int i = threadIdx.x + q * kThreads;
    wv[q] = uni_x16<OP>(x, T0 + 2 * (int64_t)(i < nwin ? i : 0), n_cols, ep, rsx);
  }
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int i = threadIdx.x + q * kThreads;
    if (i < nwin) win[i] = wv[q];
  }
  for (int i = threadIdx.x; i < 256; i += kThreads) msk[i] = i < n_pat ? pat_msk[i] : 0;
  if (tab_dinv)
    for (int i = threadIdx.x; i < n_pat; i += kThreads) dt[i] = pat_dinv[i];
  __syncthreads();
  double sq = 0.0;
#if MLAMG_UNI_PFA
#pragma unroll
#else
#pragma unroll 1
#endif
  for (int c = 0; c < CH; ++c) {
    const int64_t pr = pa + (int64_t)c * kThreads;
    const bool ok0 = 2 * pr < n_rows;
    const bool both = 2 * pr + 1 < n_rows;
    const int r = ok0 ? (int)(2 * pr) : 0;
    EpiIn u, w;
    const int64_t prn = pr + kThreads;
    if constexpr (EPF) {
      u = unx;
      w = wnx;
      if (c + 1 < CH && 2 * prn < n_rows)
        epi_load2<OP>((int)(2 * prn), 2 * prn + 1 < n_rows, ep, unx, wnx, tab_dinv, x_op);
    } else {
      if (ok0) epi_load2<OP>(r, both, ep, u, w, tab_dinv, x_op);
    }
    // the next chunk's id and far operands, in flight while this one sums
    int pnext = 0;
    dbl2 fnext[NFR];
    if constexpr (PFA) {
      if constexpr (CHA == CH) {
        const int cn = c + 1 < CHA ? c + 1 : 0;
        pnext = pall[cn];
#pragma unroll
        for (int t = 0; t < NF; ++t) fnext[t] = fall[cn][t];
      }
    }
    if constexpr (!PFA || CHA != CH) {
      pnext = (MLAMG_UNI_DBG & 2) ? 13 : pid[c + 1 < CH && 2 * prn < n_rows ? prn : 0];
#pragma unroll
      for (int t = 0; t < NF; ++t)
        fnext[t] = (MLAMG_UNI_DBG & 4) ? dbl2{0.0, 0.0}
                                       : uni_x16<OP>(x, 2 * prn + MLAMG_FAR_OFF(t, prn), n_cols, ep, rsx);
    }
    const int pl = c * kThreads + (int)threadIdx.x + hw;  // this pair's window slot
    const dbl2 xc = win[pl];
    const dbl2 xl = win[pl - 1];
    const dbl2 xr = win[pl + 1];
    const int m = msk[pcur];
    if (tab_dinv) {
      const dbl2 d = dt[pcur];
      u.c = d.x;
      w.c = d.y;
    }
    if (x_op) {
      u.b = xc.x;
      w.b = xc.y;
    }
    double s0 = 0.0, s1 = 0.0;
    int tf = 0;
#pragma unroll
    for (int q = 0; q < kRpUniMax; ++q) {
      if (q < K) {
        const int kd = uni_kind<LY>(U, q);
        double t0, t1;
        if (kd == 0) {
          const dbl2 v = win[pl + (U.off[q] >> 1)];
          t0 = v.x;
          t1 = v.y;
        } else if (kd == 1) {
          t0 = xl.y;
          t1 = xc.x;
        } else if (kd == 2) {
          t0 = xc.y;
          t1 = xr.x;
        } else {
          const dbl2 f = NF > 1 && tf == 1 ? fcur[NFR - 1] : fcur[0];
          t0 = f.x;
          t1 = f.y;
          ++tf;
        }
        const double y0 = (MLAMG_UNI_DBG & 1) || ((m >> q) & 1) ? t0 : 0.0;
        const double y1 = (MLAMG_UNI_DBG & 1) || ((m >> (q + 8)) & 1) ? t1 : 0.0;
        s0 += U.v0[q] * y0;
        s1 += U.v1[q] * y1;
      }
    }
    if (MLAMG_UNI_DBG & 8) {
      if (s0 == 1.2345 && s1 == 5.4321 && ok0) sq += epi_store2<OP>(r, both, s0, s1, u, w, ep);
    } else if (ok0) {
      sq += epi_store2<OP>(r, both, s0, s1, u, w, ep);
    }
    pcur = pnext;
#pragma unroll
    for (int t = 0; t < NF; ++t) fcur[t] = fnext[t];
  }
  if constexpr (NORM) {
    const double t = block_sum<kThreads>(sq, red);
    if (threadIdx.x == 0) ep.partial[lb] = t;
  }
#undef MLAMG_FAR_OFF
}

// ---------------------------------------------------------------- plane-marching stencil form
// k_rowpat_march: k_rowpat_uni for the 3-D 7-point layout (slots -F -n -1 0 1 n F, F = one grid
// plane of rows, even) with the far operands from LDS as well. A workgroup owns a tile of
// T = 2 CH 256 consecutive rows of a plane (rows j T .. j T + T - 1 of every plane, the last
// tile of a plane partial) and marches it through a segment of planes k0 .. k1 - 1 (2.5-D
// blocking): a ring of three LDS windows holds x around the tile in planes k - 1, k, k + 1
// (each T rows + the in-plane halo), so x[r -+ F] is the same slot of the neighbouring window
// and each row of x comes from HBM about once (plus the halo, shared with the neighbouring
// tiles that march beside it in the same XCD's L2, and two extra planes per segment), where
// k_rowpat_uni loads every far operand again (C4 A_0: 1.4x the algorithmic bytes through the
// fabric, rocprofv3 PMC). The window of plane k + 2 is loaded into registers while plane k is
// summed (plain loads survive the barrier). Per row pair: the same pattern id, mask, values,
// products and order as k_rowpat_uni — the same bits. No NORM form: the norm partials follow
// the 2048-row blocks of the other row-pair kernels, which plane tiles do not align with.
template <int OP, int CH, int PF>
__global__ __launch_bounds__(kThreads) void k_rowpat_march(
    const uint8_t* __restrict__ pid, const uint16_t* __restrict__ pat_msk, int n_pat,
    int64_t n_rows, const double* __restrict__ dinv_att, const dbl2* __restrict__ pat_dinv,
    RpUni U, const double* __restrict__ x, Epi ep, int64_t F, int nt, int seg,
    int64_t n_planes) {
  // LDS: ring[3][W] (dbl2) | dinv[n_pat] (dbl2) | mask[256] (uint16)
  extern __shared__ dbl2 uni_lds[];
  if (ep.done && *ep.done) return;
  constexpr int T = 2 * CH * kThreads;  // rows per tile
  const int hw = U.halo >> 1;           // halo in pairs
  const int W = CH * kThreads + 2 * hw;  // window slots
  dbl2* ring = uni_lds;
  dbl2* dt = ring + 3 * W;
  uint16_t* msk = reinterpret_cast<uint16_t*>(dt + n_pat);
  const bool tab_dinv = ep.dinv != nullptr && ep.dinv == dinv_att;
  bool x_op = false;
  if constexpr (OP == EPI_JACOBI || OP == EPI_JACEXP) x_op = ep.xin == x;
  if constexpr (OP == EPI_RESID) x_op = ep.copy_to != nullptr && ep.copy_from == x;
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int j = (int)(lb % nt);
  const int64_t k0 = (lb / nt) * seg;
  const int64_t k1 = k0 + seg < n_planes ? k0 + seg : n_planes;
  if (k0 >= k1) return;  // uniform per workgroup, before any barrier
  const int64_t tile0 = (int64_t)j * T;
  const int64_t lim = F - tile0;  // rows of the tile inside its plane (even)
  constexpr int WQ = CH + 2;      // window slots per thread (halo <= 256 pairs a side)
  auto wload = [&](dbl2 (&v)[WQ], int64_t k) {
    const int64_t w0 = k * F + tile0 - U.halo;
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int i = threadIdx.x + q * kThreads;
      v[q] = x16(x, w0 + 2 * (int64_t)(i < W ? i : 0), n_rows);
    }
  };
  auto wstore = [&](const dbl2 (&v)[WQ], int slot) {
    dbl2* w = ring + slot * W;
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int i = threadIdx.x + q * kThreads;
      if (i < W) w[i] = v[q];
    }
  };
  // PF planes ahead in registers: set A holds plane k + 1 at step k (k - k0 even), set B at the
  // odd steps (PF = 1: one set, reloaded every step)
  dbl2 wa[WQ], wb[WQ];
  // prologue: planes k0 - 1 and k0 staged, k0 + 1 (and k0 + 2) in flight
  wload(wa, k0 - 1);
  wstore(wa, 0);
  wload(wa, k0);
  wstore(wa, 1);
  wload(wa, k0 + 1);
  if (PF == 2 && k0 + 2 <= k1) wload(wb, k0 + 2);
  for (int i = threadIdx.x; i < 256; i += kThreads) msk[i] = i < n_pat ? pat_msk[i] : 0;
  if (tab_dinv)
    for (int i = threadIdx.x; i < n_pat; i += kThreads) dt[i] = pat_dinv[i];
  int sm = 0;  // ring slot of plane k - 1 (k, k + 1 follow cyclically)
  auto step = [&](int64_t k, dbl2 (&cur)[WQ]) {
    const int sc = sm == 2 ? 0 : sm + 1, sp = sc == 2 ? 0 : sc + 1;
    wstore(cur, sp);  // plane k + 1 (its slot held plane k - 2, last read before the last barrier)
    // this plane's pattern ids and epilogue operands, in flight across the barrier
    const int64_t rb = k * F + tile0;
    int pc[CH];
    EpiIn u[CH], w[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int lp = 2 * (c * kThreads + (int)threadIdx.x);
      const int64_t r = rb + lp;
      const bool ok0 = lp < lim && r < n_rows;
      pc[c] = ok0 ? pid[r >> 1] : 0;
      if (ok0) epi_load2<OP>((int)r, r + 1 < n_rows, ep, u[c], w[c], tab_dinv, x_op);
    }
    __syncthreads();
    // plane k + 1 + PF's window into the set just stored, in flight while PF planes sum
    if (k + 1 + PF <= k1) wload(cur, k + 1 + PF);
    const dbl2* wm = ring + sm * W;
    const dbl2* wc = ring + sc * W;
    const dbl2* wp = ring + sp * W;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int lp = 2 * (c * kThreads + (int)threadIdx.x);
      const int64_t r = rb + lp;
      if (!(lp < lim && r < n_rows)) continue;
      const bool both = r + 1 < n_rows;
      const int pl = c * kThreads + (int)threadIdx.x + hw;
      const dbl2 xc = wc[pl];
      const dbl2 xl = wc[pl - 1];
      const dbl2 xr = wc[pl + 1];
      const dbl2 fm = wm[pl];
      const dbl2 fp = wp[pl];
      const int m = msk[pc[c]];
      if (tab_dinv) {
        const dbl2 d = dt[pc[c]];
        u[c].c = d.x;
        w[c].c = d.y;
      }
      if (x_op) {
        u[c].b = xc.x;
        w[c].b = xc.y;
      }
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const int kd = uni_kind<1>(U, q);
        double t0, t1;
        if (kd == 0) {
          const dbl2 v = wc[pl + (U.off[q] >> 1)];
          t0 = v.x;
          t1 = v.y;
        } else if (kd == 1) {
          t0 = xl.y;
          t1 = xc.x;
        } else if (kd == 2) {
          t0 = xc.y;
          t1 = xr.x;
        } else {
          const dbl2 f = q == 0 ? fm : fp;
          t0 = f.x;
          t1 = f.y;
        }
        const double y0 = (m >> q) & 1 ? t0 : 0.0;
        const double y1 = (m >> (q + 8)) & 1 ? t1 : 0.0;
        s0 += U.v0[q] * y0;
        s1 += U.v1[q] * y1;
      }
      epi_store2<OP>((int)r, both, s0, s1, u[c], w[c], ep);
    }
    __syncthreads();  // plane k - 1's slot is refilled next
    sm = sc;
  };
  if constexpr (PF == 1) {
#pragma unroll 1
    for (int64_t k = k0; k < k1; ++k) step(k, wa);
  } else {
#pragma unroll 1
    for (int64_t k = k0; k < k1; k += 2) {
      step(k, wa);
      if (k + 1 < k1) step(k + 1, wb);
    }
  }
}

// Row-pair patterns with LDS row windows (C4 A_0: the x gathers, not HBM, bound k_rowpair —
// 7 16-byte loads per pair through the texture path, 36-38 us; tools/stencil_lab.hip: a 216^3
// 7-point stencil 32.6 us with every neighbour a global load, 24.4 us with x staged per
// workgroup, against 23.2 us for a copy of x into y). A workgroup owns NT pairs (rows
// [R0, R0 + 2 NT)); the wide entries' offsets form <= kRpWinMax clusters (C4: -n^2 | -n..n |
// +n^2), and for each cluster the rows of x the workgroup's pairs read through it are staged in
// LDS with 16-byte loads, all issued up front. The sums then read every operand from LDS; x is
// kept as two arrays of the even and the odd window rows (8-byte reads of one array at a
// 16-byte lane stride had 4.4 M bank conflicts per C4 pass). Values, masks and order are
// k_rowpair's, so the bits are scipy's; an epilogue operand equal to x (Jacobi's xin, the fused
// sweep's copy_from) is read from the window too. Edge pairs keep the global-load path.
// One wave's lanes of pattern p (uniform): its entries' records and values are scalar loads,
// all issued before the first is used (an SMEM result is waited for with lgkmcnt(0), which
// drains the window reads too). An entry of the staged cluster reads its two x values from the
// window (row lr + woff); the others (flag 8, at most kRpWinG per step: C4's +-n^2) are 16-byte
// global loads issued first into kRpWinG registers; each value is masked and the products are
// added in the pattern's (CSR) order.
template <int K>
__device__ __forceinline__ void rowpair_win_uniform(int p, const int32_t* pst,
                                                    const int4* __restrict__ pat_of,
                                                    const dbl2* __restrict__ pat_vv,
                                                    __amdgpu_buffer_rsrc_t rs, int r,
                                                    const double* __restrict__ we,
                                                    const double* __restrict__ wo, int lr,
                                                    double& s0, double& s1) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int a = __builtin_amdgcn_readfirstlane(pst[p]);
  const int len = __builtin_amdgcn_readfirstlane(pst[p + 1]) - a;
  const int* fi = reinterpret_cast<const int*>(pat_of);  // (offset, -, -, flags | woff << 8)
  for (int k = 0; k < len; k += K) {
    int fl[K], fo[K];
    double v0[K], v1[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
      fl[q] = __builtin_amdgcn_readfirstlane(fi[4 * (a + k + q) + 3]);
      fo[q] = __builtin_amdgcn_readfirstlane(fi[4 * (a + k + q)]);
      const dbl2 v = pat_vv[a + k + q];
      v0[q] = v.x;
      v1[q] = v.y;
    }
    // the step's global entries (scalar bookkeeping): entry qg[t] goes to register g[t]; an
    // unused register reads an out-of-range slot (zeros)
    int qg[kRpWinG], og[kRpWinG];
#pragma unroll
    for (int t = 0; t < kRpWinG; ++t) {
      qg[t] = -1;
      og[t] = 0;
    }
    {
      int t = 0;
#pragma unroll
      for (int q = 0; q < K; ++q)
        if (fl[q] & 8) {
#pragma unroll
          for (int u2 = 0; u2 < kRpWinG; ++u2)
            if (u2 == t) {
              qg[u2] = q;
              og[u2] = fo[q];
            }
          ++t;
        }
    }
    u32x4 g[kRpWinG];
#pragma unroll
    for (int t = 0; t < kRpWinG; ++t)
      g[t] = __builtin_amdgcn_raw_buffer_load_b128(
          rs, qg[t] >= 0 ? (uint32_t)(r + og[t]) * 8u : ~15u, 0, 0);
    double x0[K], x1[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
      // window row m (parity = the entry's woff parity, lr is even): even m is
      // (we[m/2], wo[m/2]), odd m (wo[m/2], we[m/2 + 1]); base pointers selected, one read
      // each (a branch per parity made the compiler wait for every earlier LDS read)
      const int wf = (fl[q] & 8) ? 0 : fl[q] >> 8;
      const int odd = wf & 1;
      const double* b0 = odd ? wo : we;
      const double* b1 = odd ? we : wo;
      const int j = (lr + wf) >> 1;
      x0[q] = b0[j];
      x1[q] = b1[j + odd];
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
      double t0 = x0[q], t1 = x1[q];
#pragma unroll
      for (int t = 0; t < kRpWinG; ++t)
        if (qg[t] == q) {  // scalar condition
          t0 = __builtin_bit_cast(double, (uint64_t)g[t].x | ((uint64_t)g[t].y << 32));
          t1 = __builtin_bit_cast(double, (uint64_t)g[t].z | ((uint64_t)g[t].w << 32));
        }
      // an entry a row does not have: +0.0 (its value is 0.0 too), as in rowpair_sums
      const double y0 = (fl[q] & 1) ? t0 : 0.0;
      const double y1 = (fl[q] & 2) ? t1 : 0.0;
      s0 += v0[q] * y0;
      s1 += v1[q] * y1;
    }
  }
}

template <int OP, bool NORM, int K>
__global__ __launch_bounds__(kRpWinNT) void k_rowpair_win(const uint16_t* __restrict__ slot,
                                                          const int32_t* __restrict__ pat_ptr,
                                                          const int4* __restrict__ pat_of,
                                                          const dbl2* __restrict__ pat_vv,
                                                          int64_t n_rows, int64_t n_cols,
                                                          const double* __restrict__ dinv_att,
                                                          const dbl2* __restrict__ pat_dinv,
                                                          RpWin W, const double* __restrict__ x,
                                                          Epi ep) {
  constexpr int NT = kRpWinNT;
  // LDS: even / odd window rows we[W.rows / 2], wo[W.rows / 2]
  extern __shared__ double rp_win_lds[];
  __shared__ double red[NT / 64];
  __shared__ int32_t pst[257];  // pattern starts
  if (ep.done && *ep.done) return;
  const int half = W.rows >> 1;
  double* we = rp_win_lds;
  double* wo = we + half;
  const bool tab_dinv = ep.dinv != nullptr && ep.dinv == dinv_att;
  bool x_op = false;  // the epilogue's x operand is x itself, in the window
  if constexpr (OP == EPI_JACOBI || OP == EPI_JACEXP) x_op = ep.xin == x && W.woff0 >= 0;
  if constexpr (OP == EPI_RESID)
    x_op = ep.copy_to != nullptr && ep.copy_from == x && W.woff0 >= 0;
  const int64_t lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t R0 = lb * 2 * NT;
  const int64_t sl = lb * NT + threadIdx.x;
  const int n_pairs_blk = (int)min<int64_t>(NT, (n_rows + 1) / 2 - lb * NT);
  const bool live = threadIdx.x < n_pairs_blk;
  // windows: 16-byte buffer loads, slots before row 0 or past n_cols read zeros; issued first
  // (they need nothing but the block index), before the slot load and the epilogue loads that
  // depend on it, and all before the first LDS store
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(n_cols * 8), 0x00020000);
  auto wload = [&](int i) {
    const int t = 2 * i;
    int k = 0;
#pragma unroll
    for (int c = 1; c < kRpWinMax; ++c) k += (c < W.n && t >= W.base[c]) ? 1 : 0;
    const int64_t g = R0 + W.s[k] + (t - W.base[k]);
    return __builtin_amdgcn_raw_buffer_load_b128(rs, g >= 0 ? (uint32_t)(g * 8) : ~15u, 0, 0);
  };
  auto wstore = [&](int i, const u32x4& t) {
    we[i] = __builtin_bit_cast(double, (uint64_t)t.x | ((uint64_t)t.y << 32));
    wo[i] = __builtin_bit_cast(double, (uint64_t)t.z | ((uint64_t)t.w << 32));
  };
#ifndef MLAMG_RPW_DBG  // timing variants only (tools/build_variant.sh): 1 no sums, 2 no staging
#define MLAMG_RPW_DBG 0
#endif
  constexpr int WQ = 4;  // slots per thread in registers (C4: 3.9 with every cluster staged)
  u32x4 wv[WQ];
  if (!(MLAMG_RPW_DBG & 2)) {
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int i = threadIdx.x + q * NT;
      if (i < half) wv[q] = wload(i);
    }
  }
  const int sv = live ? (int)slot[sl] : 0;
  const int p = sv & 0xff;
  const int64_t pr = lb * NT + (sv >> 8);
  const bool both = 2 * pr + 1 < n_rows;
  const int r = (int)(2 * pr);
  EpiIn u, w;
  if (live) epi_load2<OP>(r, both, ep, u, w, tab_dinv, x_op);
  dbl2 dv = {0.0, 0.0};
  if (live && tab_dinv) dv = pat_dinv[p];
  if (!(MLAMG_RPW_DBG & 2)) {
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int i = threadIdx.x + q * NT;
      if (i < half) wstore(i, wv[q]);
    }
    for (int i = threadIdx.x + WQ * NT; i < half; i += NT) wstore(i, wload(i));
  }
  for (int i = threadIdx.x; i < 257; i += NT) pst[i] = pat_ptr[i];
  __syncthreads();
  double sq = 0.0;
  if (live) {
    if (tab_dinv) {
      u.c = dv.x;
      w.c = dv.y;
    }
    const int lr = (int)(r - R0);
    if (x_op) {  // window row lr + woff0 (even: lr and woff0 are)
      const int j = (lr + W.woff0) >> 1;
      u.b = we[j];
      w.b = both ? wo[j] : 0.0;
    }
  }
  // one pass per distinct pattern of the wave (sorted slots: one, at a pattern boundary two or
  // three), the pattern's records as scalar loads. Every pair reads its operands from the
  // windows, the matrix's first and last pairs too: rows outside x were staged as zeros and
  // are masked like every entry a row does not have.
  double s0 = 0.0, s1 = 0.0;
  uint64_t todo = (MLAMG_RPW_DBG & 1) ? 0 : __ballot(live);
  while (todo) {
    const int p0 = __builtin_amdgcn_readlane(p, (int)__builtin_ctzll(todo));
    const bool mine = live && p == p0;
    todo &= ~__ballot(mine);
    if (mine)
      rowpair_win_uniform<K>(p0, pst, pat_of, pat_vv, rs, r, we, wo, (int)(r - R0), s0, s1);
  }
  if (live && !(MLAMG_RPW_DBG & 4)) sq = epi_store2<OP>(r, both, s0, s1, u, w, ep);
  if constexpr (NORM) {
    const double t = block_sum<NT>(sq, red);
    if (threadIdx.x == 0) ep.partial[lb] = t;
  }
}

// ---------------------------------------------------------------- CSR-vector (canonical order)
// Lane-parallel sums for long rows (coarse Galerkin operators A_l, R = P^T: hundreds of entries
// per row, where a one-lane left-to-right chain costs ~15-25 cycles per entry: tools/
// chain_lab.hip). Every width W = 64 Q (Q = 1, 2, 4, 8 waves per row) computes the SAME
// canonical order — the order of 512 virtual lanes:
//   virtual lane v = 64 w + l (w = 0..7, l = 0..63) sums the row's entries v, v + 512, ... left
//   to right from +0.0; each virtual wave w folds its 64 lanes with an xor butterfly (off = 32
//   .. 1); the row is ((ws_0 + ws_1) + ...) + ws_7.
// Physical wave p of a row (0..Q-1) holds the virtual waves w = p + Q j (j < 8 / Q), one
// accumulator each. An empty virtual lane holds +0.0, which no butterfly step or wave sum can
// see (a sum started at +0.0 is never -0.0). So the width is a pure performance choice: every
// W gives the same bits (oracle.c vec_matvec restates the order; VERDICT r02 item 2 — the
// autotune's timing noise used to pick between lane-strided orders).
// Residual norms are written per row (partial[row]), so the norm is width-independent too.
#ifndef MLAMG_VCAN_STEPS  // A/B knob: 512-entry stripes per wave per step, times Q
#define MLAMG_VCAN_STEPS 1
#endif
constexpr int kVcanSteps = MLAMG_VCAN_STEPS;
template <int Q, int OP, bool NORM, typename IT>
__global__ __launch_bounds__(512) void k_csr_vcan(const int32_t* __restrict__ indptr,
                                                  const IT* __restrict__ indices,
                                                  const double* __restrict__ vals,
                                                  int64_t n_rows, const double* __restrict__ x,
                                                  Epi ep) {
  constexpr int J = 8 / Q;    // virtual waves per physical wave (accumulators per lane)
  constexpr int RPB = 8 / Q;  // rows per 512-thread workgroup
  __shared__ double ws[RPB][8];
  if (ep.done && *ep.done) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rloc = wave / Q, p = wave % Q;
  const int64_t row = (int64_t)blockIdx.x * RPB + rloc;
  double acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = 0.0;
  EpiIn pre;
  const bool head = p == 0 && lane == 0 && row < n_rows;
  if (head) pre = epi_load<OP>((int)row, ep);
  if (row < n_rows) {
    const int a = indptr[row], b = indptr[row + 1];
    // T = S Q stripes of 512 entries per step: 8 S entries per lane in flight
    constexpr int T = kVcanSteps * Q;
    for (int base = a; base < b; base += 512 * T) {
      int32_t cc[T][J];
      double vv[T][J], xv[T][J];
      if (ep.cached) {  // uniform: one unrolled load sequence or the other
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const int e = base + 512 * t + 64 * (p + Q * j) + lane;
            cc[t][j] = e < b ? (int32_t)indices[e] : -1;
            vv[t][j] = e < b ? vals[e] : 0.0;
          }
      } else {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const int e = base + 512 * t + 64 * (p + Q * j) + lane;
            cc[t][j] = e < b ? (int32_t)__builtin_nontemporal_load(indices + e) : -1;
            vv[t][j] = e < b ? __builtin_nontemporal_load(vals + e) : 0.0;
          }
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int j = 0; j < J; ++j) xv[t][j] = cc[t][j] >= 0 ? x[cc[t][j]] : 0.0;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (cc[t][j] >= 0) acc[j] += vv[t][j] * xv[t][j];
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < J; ++j) ws[rloc][p + Q * j] = acc[j];
  __syncthreads();
  if (head) {
    double r = ws[rloc][0];
#pragma unroll
    for (int w = 1; w < 8; ++w) r += ws[rloc][w];
    const double sq = epi_store<OP>((int)row, r, pre, ep);
    if constexpr (NORM) ep.partial[row] = sq;
  }
}

template <int OP, bool NORM, int Q>
static int launch_vcan(const mlamg_csr* A, const double* x, const Epi& ep, hipStream_t s) {
  constexpr int RPB = 8 / Q;
  const unsigned nb = (unsigned)std::max<int64_t>(1, (A->n_rows + RPB - 1) / RPB);
  if (A->vec_idx16)
    MLAMG_LAUNCH((k_csr_vcan<Q, OP, NORM, uint16_t>), dim3(nb), dim3(512), 0, s, A->indptr,
                       A->vec_idx16, A->data, A->n_rows, x, ep);
  else
    MLAMG_LAUNCH((k_csr_vcan<Q, OP, NORM, int32_t>), dim3(nb), dim3(512), 0, s, A->indptr,
                       A->indices, A->data, A->n_rows, x, ep);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// The same canonical order for the long-row coarse operators where k_csr_vcan is latency-bound
// (C4 level 3: 10,078 rows of ~709 entries; a 512-thread workgroup per 1-2 rows issues its loads
// once and drains: 22-27 us for a 71 MB stream; a wave that walks whole rows one after another
// pays a chain of memory round trips per row instead). A 1024-thread workgroup owns a contiguous
// range of rows (their bounds staged in LDS), dealt to its 16 waves. A wave walks its rows'
// 512-entry stripes (virtual wave j of a stripe = entry 64 j + lane, one accumulator each) as a
// software pipeline: the loads of the next stripe are in flight while the current one is
// gathered and summed, across row ends too. x is staged in LDS once per workgroup when it fits
// (XL), so the gathers leave the texture address unit (TA busy 51 % on A_3 with x gathered from
// L2). Bitwise k_csr_vcan's order at every width: entry e of a row goes to
// virtual lane (e - start) mod 512 and each virtual lane sums its entries left to right.
constexpr int kVwThreads = 1024;
constexpr int64_t kVwMaxX = 16384;     // doubles of x in LDS (128 KiB)
constexpr int64_t kVwMaxRows = 4096;   // rows per workgroup (bounds in LDS, 16 KiB)

// one stripe of a wave: 8 entries per lane (virtual waves j = 0..7), every load unconditional
// (buffer loads, out-of-range offsets read 0) and masked by selects, so the loop body has no
// divergent branch and the compiler's wait counts keep the next stripe's loads in flight
struct VwStripe {
  int32_t c[8];
  double v[8];
  EpiIn pre;  // epilogue operands of the stripe's row (loaded with every stripe: same lines)
  int row;    // local row
  int e0, lb; // stripe start and row end: the mask is applied when the stripe is consumed (a
              // select right after the load would wait for it)
  bool last;  // last stripe of the row
};

template <int OP, bool NORM, typename IT, bool XL, bool NT>
__global__ __launch_bounds__(kVwThreads) void k_vcan_wave(const int32_t* __restrict__ indptr,
                                                          const IT* __restrict__ indices,
                                                          const double* __restrict__ vals,
                                                          int64_t n_rows, int64_t n_cols,
                                                          int64_t nnz, int64_t rows_per_block,
                                                          const double* __restrict__ x, Epi ep) {
  extern __shared__ double lds[];
  if (ep.done && *ep.done) return;
  constexpr int kAux = NT ? 2 : 0;  // nt: non-temporal stream (see kCachedNnz)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int nr = (int)min<int64_t>(rows_per_block, n_rows - r0);
  const int64_t xw = XL ? ((n_cols + 1) & ~int64_t(1)) : 0;
  int32_t* rp = reinterpret_cast<int32_t*>(lds + xw);
  for (int i = threadIdx.x; i <= nr; i += kVwThreads) rp[i] = indptr[r0 + i];
  if constexpr (XL) {
    for (int64_t i = threadIdx.x; i < n_cols; i += 8 * kVwThreads) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = i + u * kVwThreads;
        v[u] = k < n_cols ? x[k] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = i + u * kVwThreads;
        if (k < n_cols) lds[k] = v[u];
      }
    }
  }
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rsI =
      __builtin_amdgcn_make_buffer_rsrc((void*)indices, 0, (int)(nnz * sizeof(IT)), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV =
      __builtin_amdgcn_make_buffer_rsrc((void*)vals, 0, (int)(nnz * 8), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsX =
      __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(n_cols * 8), 0x00020000);
  // load cursor (wave-uniform): row lr (local), its bounds [la, lb), next stripe start le; a row
  // of any length (empty included) is at least one stripe; past the last row the cursor reads
  // an empty range
  int lr = wave;
  if (lr >= nr) return;
  int la = __builtin_amdgcn_readfirstlane(rp[lr]);
  int lb = __builtin_amdgcn_readfirstlane(rp[lr + 1]);
  int le = la;
  auto load = [&](VwStripe& s) {
    s.row = lr;
    s.e0 = le;
    s.lb = lb;
    s.last = le + 512 >= lb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = le + 64 * j + lane;
      if constexpr (sizeof(IT) == 2)
        s.c[j] = (int32_t)__builtin_amdgcn_raw_buffer_load_b16(rsI, e * 2, 0, kAux);
      else
        s.c[j] = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rsI, e * 4, 0, kAux);
      s.v[j] =
          __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsV, e * 8, 0, kAux));
    }
    s.pre = epi_load<OP>((int)min<int64_t>(r0 + lr, n_rows - 1), ep);
    le += 512;
    if (le >= lb) {
      lr += kVwThreads / 64;
      const bool in = lr < nr;
      la = in ? __builtin_amdgcn_readfirstlane(rp[lr]) : 0;
      lb = in ? __builtin_amdgcn_readfirstlane(rp[lr + 1]) : 0;
      le = la;
    }
  };
  double acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  auto gather = [&](const VwStripe& s, double* xv) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = s.e0 + 64 * j + lane < s.lb;
      if constexpr (XL)
        xv[j] = lds[ok ? s.c[j] : 0];
      else  // past the row: offset 0xfffffff8, out of range, reads 0
        xv[j] = __builtin_bit_cast(
            double, __builtin_amdgcn_raw_buffer_load_b64(rsX, ok ? (uint32_t)s.c[j] * 8u : ~7u,
                                                         0, 0));
    }
  };
  auto sum = [&](const VwStripe& s, const double* xv) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc[j] = s.e0 + 64 * j + lane < s.lb ? acc[j] + s.v[j] * xv[j] : acc[j];
    if (s.last) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
      if (lane == 0) {
        double r = acc[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) r += acc[j];
        const double sq = epi_store<OP>((int)(r0 + s.row), r, s.pre, ep);
        if constexpr (NORM) ep.partial[r0 + s.row] = sq;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    }
  };
  // x in LDS: issue the next stripe's loads, then gather and sum this one; x in memory: gather
  // this one first (vmcnt is in order: its gathers must not queue behind the next stripe)
  auto step = [&](VwStripe& cur, VwStripe& nxt) -> bool {
    double xv[8];
    const bool more = lr < nr;
    if constexpr (XL) {
      load(nxt);
      gather(cur, xv);
    } else {
      gather(cur, xv);
      load(nxt);
    }
    sum(cur, xv);
    return more;
  };
  VwStripe sa, sb;
  load(sa);
  while (step(sa, sb) && step(sb, sa)) {
  }
}

static int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

// MLAMG_VCAN_WAVE=1 takes k_vcan_wave (x in LDS when it fits), =2 without the LDS copy of x;
// unset / 0 keeps k_csr_vcan, which measured as fast or faster on every C4 operator.
// Read at every launch (a host getenv, not a device cost) so one process can compare them.
static int vcan_wave_mode() {
  const char* e = std::getenv("MLAMG_VCAN_WAVE");
  return e ? std::atoi(e) : 0;
}

template <int OP, bool NORM, typename IT, bool XL>
static void launch_vcan_wave_nt(const mlamg_csr* A, const IT* idx, const double* x,
                                const Epi& ep, hipStream_t s, unsigned nb, size_t lds,
                                int64_t rpb) {
  if (ep.cached)
    MLAMG_LAUNCH((k_vcan_wave<OP, NORM, IT, XL, false>), dim3(nb), dim3(kVwThreads), lds, s,
                       A->indptr, idx, A->data, A->n_rows, A->n_cols, A->nnz, rpb, x, ep);
  else
    MLAMG_LAUNCH((k_vcan_wave<OP, NORM, IT, XL, true>), dim3(nb), dim3(kVwThreads), lds, s,
                       A->indptr, idx, A->data, A->n_rows, A->n_cols, A->nnz, rpb, x, ep);
}

template <int OP, bool NORM, typename IT>
static void launch_vcan_wave(const mlamg_csr* A, const IT* idx, const double* x, const Epi& ep,
                             hipStream_t s) {
  const bool xl = A->n_cols <= kVwMaxX && vcan_wave_mode() != 2;
  // one workgroup per CU with x in LDS (up to 144 KiB with the row bounds); two without
  const int64_t slots = (int64_t)device_cus() * (xl ? 1 : 2);
  const int64_t rpb = std::min<int64_t>(kVwMaxRows,
                                        std::max<int64_t>(1, (A->n_rows + slots - 1) / slots));
  const unsigned nb = (unsigned)((A->n_rows + rpb - 1) / rpb);
  const size_t rows_lds = sizeof(int32_t) * (size_t)(rpb + 1);
  if (xl)
    launch_vcan_wave_nt<OP, NORM, IT, true>(
        A, idx, x, ep, s, nb, sizeof(double) * ((A->n_cols + 1) & ~int64_t(1)) + rows_lds, rpb);
  else
    launch_vcan_wave_nt<OP, NORM, IT, false>(A, idx, x, ep, s, nb, rows_lds, rpb);
}

template <int OP, bool NORM>
static int launch_vec(const mlamg_csr* A, const double* x, const Epi& ep, hipStream_t s) {
  if (A->n_rows == 0) return MLAMG_OK;
  // buffer offsets are 32-bit: the wave kernel takes streams below 2 GiB
  if (vcan_wave_mode() != 0 && A->nnz < (int64_t(1) << 28) && A->n_cols < (int64_t(1) << 28)) {
    if (A->vec_idx16)
      launch_vcan_wave<OP, NORM, uint16_t>(A, A->vec_idx16, x, ep, s);
    else
      launch_vcan_wave<OP, NORM, int32_t>(A, A->indices, x, ep, s);
    MLAMG_HIP(hipGetLastError());
    return MLAMG_OK;
  }
  switch (A->vec_width) {
    case 128: return launch_vcan<OP, NORM, 2>(A, x, ep, s);
    case 256: return launch_vcan<OP, NORM, 4>(A, x, ep, s);
    case 512: return launch_vcan<OP, NORM, 8>(A, x, ep, s);
    default: return launch_vcan<OP, NORM, 1>(A, x, ep, s);
  }
}

// Left-to-right sum of p[ka..kb) by one lane. Measured (tools/chain_lab.hip, MI355X): a
// dependent v_add_f64 chain costs ~14-17 cycles per element at best; an LDS read waited for
// per element ~85, per batch of 8 ~26-33, of 32 ~17-28 — so batches of 32 reads, then 32 adds
// (software pipelining across batches loses: the register copies between the buffers wait for
// the fresh reads at the end of every iteration).
// Batches of 16 (round 3): the 32-read batch needed 64 VGPRs for the batch alone, so the
// sorted kernel's long-row instantiation (R_1, A_2, P_3 on C4) ran at 80-92 VGPRs, 5 waves per
// SIMD, i.e. 2 resident 512-thread blocks per CU instead of 4: with 16 it fits 55-60 VGPRs, and
// the C4 cycle went 0.80 -> 0.77 ms (same box, alternating: 1,225-1,253 -> 1,288-1,307 V-cycles/s).
#ifndef MLAMG_CHAIN_BATCH  // build-time A/B knob: LDS reads per batch (registers: 2 per read)
#define MLAMG_CHAIN_BATCH 16
#endif
__device__ __forceinline__ double chain_sum(const double* __restrict__ p, int ka, int kb,
                                            double s) {
  constexpr int CB = MLAMG_CHAIN_BATCH;
  int k = ka;
  for (; k + CB <= kb; k += CB) {
    double v[CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) v[u] = p[k + u];
#pragma unroll
    for (int u = 0; u < CB; ++u) s += v[u];
  }
  for (; k + 8 <= kb; k += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[k + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  // the last < 8 entries: all reads issued together (the index is clamped to the row's last
  // entry, so no read leaves the row), then the adds that belong to the row, in order
  const int rem = kb - k;
  if (rem > 0) {
    double v[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) v[u] = p[k + min(u, rem - 1)];
#pragma unroll
    for (int u = 0; u < 7; ++u) s = u < rem ? s + v[u] : s;
  }
  return s;
}

// Two rows' left-to-right sums at once: batches of 8 reads from each row, then the 16 adds
// alternating between the two chains (independent, so each hides the other's add latency);
// each row's products are added in stored order.
__device__ __forceinline__ void sum_two_rows(const double* __restrict__ p, int a0, int b0, int a1,
                                             int b1, double& s0, double& s1) {
  while (a0 + 8 <= b0 && a1 + 8 <= b1) {
    double u[8], v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      u[k] = p[a0 + k];
      v[k] = p[a1 + k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s0 += u[k];
      s1 += v[k];
    }
    a0 += 8;
    a1 += 8;
  }
  s0 = chain_sum(p, a0, b0, s0);
  s1 = chain_sum(p, a1, b1, s1);
}

// ---------------------------------------------------------------- gather-sorted CSR-stream
// Same two phases as k_csr_stream, but each block's nonzeros are stored in ascending column
// order, packed with their CSR slot: the 64 gathers of one wave-instruction then fall on a few
// cache lines instead of one per row neighbourhood (the x gather, not HBM, bounds long-row
// operators: Galerkin A_l, R = P^T). Products are written to LDS at their CSR slot and phase 2
// sums every row in stored order, so the result is bitwise k_csr_stream's (scipy's).
// VM: how the values are stored — 0 fp64 (8 B per nonzero); 1 a <= 256-entry dictionary (one
// byte per nonzero, the table staged in LDS); 2 a dictionary per block (two bytes per nonzero
// plus the block's distinct values, read as one contiguous stream and staged in the LDS the
// products use later). The products and their order are those of the fp64 form, so every
// mode computes the same bits.
#ifndef MLAMG_SRT_BUF  // build-time A/B knob: x gathers through a buffer resource with 32-bit
#define MLAMG_SRT_BUF 1  // offsets (a padded entry reads out of range, i.e. 0) and the 2-byte value
#endif                   // codes packed two to a register: P_0 72-74.5 -> 69-70 us
#ifndef MLAMG_SRT_WAVES  // minimum waves per SIMD the register allocation must allow (0: free)
#define MLAMG_SRT_WAVES 0
#endif
template <int OP, bool NORM, int VM, bool LR>
__global__ __launch_bounds__(kSrtThreads)
__attribute__((amdgpu_waves_per_eu(MLAMG_SRT_WAVES > 0 ? MLAMG_SRT_WAVES : 1, 8)))
void k_sorted(const int32_t* __restrict__ indptr,
                                                        const uint32_t* __restrict__ pk,
                                                        const double* __restrict__ av,
                                                        const uint8_t* __restrict__ vi,
                                                        const double* __restrict__ vtab,
                                                        const uint16_t* __restrict__ vc,
                                                        const int32_t* __restrict__ vblk,
                                                        const int32_t* __restrict__ blk,
                                                        const int32_t* __restrict__ base,
                                                        const double* __restrict__ x, Epi ep) {
  constexpr bool VD = VM == 1;
  __shared__ double prod[kSrtNnz];
  __shared__ int32_t rp[kSrtRows + 1];
  __shared__ double red[kSrtThreads / 64];
  __shared__ double valt[VD ? 256 : 1];
  if (ep.done && *ep.done) return;
  const int b = (int)xcd_block(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  // every global load of the block is issued before the first LDS store that needs one (a
  // store waits for its load, and a load placed after it would wait too): the value table and
  // the row pointers go to registers first and to LDS just before the barrier
  double tv = 0.0;
  if constexpr (VD) tv = vtab[tid & 255];
  int2 dict = {0, 0};  // VM 2: the block's dictionary (offset, size), its first load
  if constexpr (VM == 2) dict = reinterpret_cast<const int2*>(vblk)[b];
  // the block's record {r0, r1, e0, nnz, lo, hi, split, -} (one 32-byte load) goes out first;
  // the entry stream is laid out at a fixed stride (formats.hip k_srt_pad: block b at
  // b * kSrtNnz, padded with kNone), so its loads need nothing from the record and follow at once, in flight while
  // the record's round trip completes (loads retire in order: the row-pointer and epilogue
  // loads that depend on the record then wait for it alone)
  const int4 m0 = reinterpret_cast<const int4*>(base)[2 * b];
  const int4 m1 = reinterpret_cast<const int4*>(base)[2 * b + 1];
  // SB: every in-range offset is below 2^31 (n_cols < 2^28, checked at build), the padding
  // offset ~7 is above the record count and reads 0
  const __amdgpu_buffer_rsrc_t rsx =
      __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, 0x7ffffff8, 0x00020000);
  constexpr int U = kSrtNnz / kSrtThreads;
  constexpr uint32_t kNone = 0xffffffffu, kSlot = (1u << kSrtPosBits) - 1;
  uint32_t w[U];
  double vv[U], xv[U];
  constexpr bool SB = MLAMG_SRT_BUF != 0;
  uint32_t cv[VM == 2 ? (SB ? U / 2 : U) : 1];  // SB: codes u and u + 1 in one register
  {
    const size_t eb = (size_t)b * kSrtNnz + tid;
    if (ep.cached) {  // uniform: one unrolled load sequence or the other
#pragma unroll
      for (int u = 0; u < U; ++u) {
        w[u] = pk[eb + u * kSrtThreads];
        if constexpr (VM == 2 && SB)
          cv[u >> 1] = (u & 1) ? cv[u >> 1] | ((uint32_t)vc[eb + u * kSrtThreads] << 16)
                               : (uint32_t)vc[eb + u * kSrtThreads];
        else if constexpr (VM == 2)
          cv[u] = vc[eb + u * kSrtThreads];
        else if constexpr (VD)
          vv[u] = (double)vi[eb + u * kSrtThreads];  // index for now
        else
          vv[u] = av[eb + u * kSrtThreads];
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        w[u] = __builtin_nontemporal_load(pk + eb + u * kSrtThreads);
        if constexpr (VM == 2 && SB)
          cv[u >> 1] = (u & 1) ? cv[u >> 1] | ((uint32_t)__builtin_nontemporal_load(
                                                   vc + eb + u * kSrtThreads) << 16)
                               : (uint32_t)__builtin_nontemporal_load(vc + eb + u * kSrtThreads);
        else if constexpr (VM == 2)
          cv[u] = __builtin_nontemporal_load(vc + eb + u * kSrtThreads);
        else if constexpr (VD)
          vv[u] = (double)__builtin_nontemporal_load(vi + eb + u * kSrtThreads);  // index for now
        else
          vv[u] = __builtin_nontemporal_load(av + eb + u * kSrtThreads);
      }
    }
  }
  if constexpr (VM == 2) {
    // the block's dictionary (<= kSrtNnz values, one contiguous run): into vv for now, to LDS
    // below
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kSrtThreads;
      vv[u] = i < dict.y ? __builtin_nontemporal_load(vtab + dict.x + i) : 0.0;
    }
  }
  const int r0 = m0.x, r1 = m0.y, nr = r1 - r0;
  const int e0 = m0.z;
  // two column windows per block: sorted entries [0, split) are offsets from lo, the rest from
  // hi (a halo-extended local matrix has its ghost columns far from the owned ones)
  const int lo = m1.x, hi = m1.y, split = m1.z;
  constexpr int RPQ = kSrtRows / kSrtThreads + 1;  // row pointers per thread (nr + 1 <= kSrtRows + 1)
  int rpv[RPQ];
#pragma unroll
  for (int q = 0; q < RPQ; ++q) {
    const int t = tid + q * kSrtThreads;
    rpv[q] = t <= nr ? indptr[r0 + t] : 0;
  }
  constexpr int RPT = kSrtRows / kSrtThreads;  // rows per thread in phase 2
  static_assert(RPT * kSrtThreads == kSrtRows, "whole rows per thread in phase 2");
  EpiIn pre[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q)
    if (tid + q * kSrtThreads < nr) pre[q] = epi_load<OP>(r0 + tid + q * kSrtThreads, ep);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int cb = tid + u * kSrtThreads < split ? lo : hi;
#ifdef MLAMG_SRT_LAB_NOGATHER  // timing variant only (tools/p0r0_time.py): no x gathers
    xv[u] = (double)(cb + (int)(w[u] >> kSrtPosBits));
#else
    if constexpr (SB) {
      const uint32_t off = w[u] != kNone ? (uint32_t)(cb + (int)(w[u] >> kSrtPosBits)) * 8u : ~7u;
      xv[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsx, off, 0, 0));
    } else {
      xv[u] = w[u] != kNone ? x[cb + (int)(w[u] >> kSrtPosBits)] : 0.0;
    }
#endif
  }
#pragma unroll
  for (int q = 0; q < RPQ; ++q) {
    const int t = tid + q * kSrtThreads;
    if (t <= nr) rp[t] = rpv[q] - e0;
  }
  if constexpr (VD) {
    if (tid < 256) valt[tid] = tv;
    __syncthreads();  // value table staged (the gathers above are already in flight)
#pragma unroll
    for (int u = 0; u < U; ++u) vv[u] = w[u] != kNone ? valt[(int)vv[u]] : 0.0;
  }
  if constexpr (VM == 2) {
    // the dictionary goes through the product array: staged, looked up, then overwritten by
    // the products after a second barrier
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * kSrtThreads;
      if (i < dict.y) prod[i] = vv[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = SB ? (int)((cv[u >> 1] >> (16 * (u & 1))) & 0xffffu) : (int)cv[u];
      vv[u] = w[u] != kNone ? prod[c] : 0.0;
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (w[u] != kNone) prod[w[u] & kSlot] = vv[u] * xv[u];
  __syncthreads();
  double sq = 0.0;
  // LR = false, short rows (P_0, R_0, A_1: 4-40 entries): one row after the other in 4-entry
  // batches. LR = true, long rows (operators averaging >= kSrtLongRow entries per row, e.g. A_3:
  // 709): the thread's two rows side by side in 8-entry batches. A separate instantiation, not a
  // branch: with both forms in one kernel the extra registers cost the short-row operators
  // 10-20 % (measured on the C4 hierarchy, tools/coarse_formats.py; the two-row form cuts
  // A_3 65 -> 34 us and R_2 33 -> 20 us)
#ifndef MLAMG_SRT_SHORT2  // A/B knob: short rows two at a time (1) or one after the other (0)
#define MLAMG_SRT_SHORT2 1
#endif
  if constexpr (!LR && MLAMG_SRT_SHORT2 && RPT == 2) {
    const int t0 = tid, t1 = tid + kSrtThreads;
    if (t0 < nr) {
      double s0 = 0.0, s1 = 0.0;
      int a0 = rp[t0];
      const int b0 = rp[t0 + 1];
      int a1 = t1 < nr ? rp[t1] : 0;
      const int b1 = t1 < nr ? rp[t1 + 1] : 0;
      while (a0 + 4 <= b0 && a1 + 4 <= b1) {
        const double p0 = prod[a0], p1 = prod[a0 + 1], p2 = prod[a0 + 2], p3 = prod[a0 + 3];
        const double q0 = prod[a1], q1 = prod[a1 + 1], q2 = prod[a1 + 2], q3 = prod[a1 + 3];
        s0 += p0;
        s1 += q0;
        s0 += p1;
        s1 += q1;
        s0 += p2;
        s1 += q2;
        s0 += p3;
        s1 += q3;
        a0 += 4;
        a1 += 4;
      }
      for (; a0 + 4 <= b0; a0 += 4) {
        const double p0 = prod[a0], p1 = prod[a0 + 1], p2 = prod[a0 + 2], p3 = prod[a0 + 3];
        s0 += p0;
        s0 += p1;
        s0 += p2;
        s0 += p3;
      }
      for (; a0 < b0; ++a0) s0 += prod[a0];
      for (; a1 + 4 <= b1; a1 += 4) {
        const double q0 = prod[a1], q1 = prod[a1 + 1], q2 = prod[a1 + 2], q3 = prod[a1 + 3];
        s1 += q0;
        s1 += q1;
        s1 += q2;
        s1 += q3;
      }
      for (; a1 < b1; ++a1) s1 += prod[a1];
      sq += epi_store<OP>(r0 + t0, s0, pre[0], ep);
      if (t1 < nr) sq += epi_store<OP>(r0 + t1, s1, pre[1], ep);
    }
  } else if constexpr (!LR) {
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int t = tid + q * kSrtThreads;
      if (t >= nr) break;
      double s = 0.0;
      const int ka = rp[t], kb = rp[t + 1];
      int k = ka;
      for (; k + 4 <= kb; k += 4) {
        const double p0 = prod[k], p1 = prod[k + 1], p2 = prod[k + 2], p3 = prod[k + 3];
        s += p0;
        s += p1;
        s += p2;
        s += p3;
      }
      for (; k < kb; ++k) s += prod[k];
      sq += epi_store<OP>(r0 + t, s, pre[q], ep);
    }
  } else if constexpr (RPT == 2) {
    // the thread's two rows summed side by side: two independent dependent-add chains share
    // the LDS read latency and each other's add latency (each row still left to right)
    const int t0 = tid, t1 = tid + kSrtThreads;
    if (t1 < nr) {
      double s0 = 0.0, s1 = 0.0;
      sum_two_rows(prod, rp[t0], rp[t0 + 1], rp[t1], rp[t1 + 1], s0, s1);
      sq += epi_store<OP>(r0 + t0, s0, pre[0], ep);
      sq += epi_store<OP>(r0 + t1, s1, pre[1], ep);
    } else if (t0 < nr) {
      sq += epi_store<OP>(r0 + t0, chain_sum(prod, rp[t0], rp[t0 + 1], 0.0), pre[0], ep);
    }
  } else {
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int t = tid + q * kSrtThreads;
      if (t >= nr) break;
      sq += epi_store<OP>(r0 + t, chain_sum(prod, rp[t], rp[t + 1], 0.0), pre[q], ep);
    }
  }
  if constexpr (NORM) {
    const double t = block_sum<kSrtThreads>(sq, red);
    if (tid == 0) ep.partial[b] = t;
  }
}

// ---------------------------------------------------------------- long-row CSR ("long")
// scipy's order for long rows (coarse Galerkin operators A_l and R = P^T: hundreds of nonzeros
// per row). One 256-thread workgroup per tile of <= kLongRows consecutive rows holding
// <= kLongNnz nonzeros. Phase 1 streams the tile's entries (kLongNnz / 256 per lane, every index
// and value load issued before the first gather) and writes the products to LDS. Phase 2 gives
// each row to one lane — row t to wave t % 4, lane t / 4, so the four SIMDs sum side by side —
// which adds its products left to right with the LDS reads issued eight ahead of the adds: the
// chain is then bound by the dependent fp64 adds instead of the ~50-cycle LDS latency that an
// unpipelined loop pays per read (the CSR-stream kernel on C4 level 3: 64 us). A row longer than
// kLongNnz is a tile of its own, streamed in chunks with lane 0 carrying the sum. Bitwise
// csr_matvec — unlike the lane-strided CSR-vector order this format replaces in the autotune, so
// the kernel choice (a timing decision) can no longer change a result.
template <int OP, bool NORM>
__global__ __launch_bounds__(kThreads) void k_csr_long(const int32_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices,
                                                       const double* __restrict__ vals,
                                                       const int32_t* __restrict__ tile,
                                                       const double* __restrict__ x, Epi ep) {
  __shared__ double prod[kLongNnz];
  __shared__ int32_t rp[kLongRows + 1];
  __shared__ double red[kThreads / 64];
  static_assert(kLongRows <= kThreads && kLongRows % 4 == 0, "rows spread over four waves");
  if (ep.done && *ep.done) return;
  const int b = (int)xcd_block(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  const int r0 = tile[b], r1 = tile[b + 1], nr = r1 - r0;
  const int e0 = indptr[r0];
  const int ne = indptr[r1] - e0;
  const int t = (tid & 63) * 4 + (tid >> 6);  // this lane's row in phase 2
  double sq = 0.0;
  if (ne <= kLongNnz) {
    EpiIn pre;
    if (t < nr) pre = epi_load<OP>(r0 + t, ep);
    const int rpa = tid <= nr ? indptr[r0 + tid] : 0;
    constexpr int U = kLongNnz / kThreads;
    const int32_t* ci = indices + e0;
    const double* cv = vals + e0;
    int32_t cc[U];
    double vv[U], xv[U];
    if (ep.cached) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = tid + u * kThreads;
        cc[u] = e < ne ? ci[e] : -1;
        vv[u] = e < ne ? cv[e] : 0.0;
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = tid + u * kThreads;
        cc[u] = e < ne ? __builtin_nontemporal_load(ci + e) : -1;
        vv[u] = e < ne ? __builtin_nontemporal_load(cv + e) : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xv[u] = cc[u] >= 0 ? x[cc[u]] : 0.0;
    if (tid <= nr) rp[tid] = rpa - e0;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tid + u * kThreads < ne) prod[tid + u * kThreads] = vv[u] * xv[u];
    __syncthreads();
    if (t < nr) sq += epi_store<OP>(r0 + t, chain_sum(prod, rp[t], rp[t + 1], 0.0), pre, ep);
  } else {
    // one row longer than a tile: chunks through LDS, lane 0 carries the ordered sum
    double s = 0.0;
    for (int c = 0; c < ne; c += kLongNnz) {
      const int m = min(kLongNnz, ne - c);
      for (int e = tid; e < m; e += kThreads)
        prod[e] = vals[e0 + c + e] * x[indices[e0 + c + e]];
      __syncthreads();
      if (tid == 0) s = chain_sum(prod, 0, m, s);
      __syncthreads();
    }
    if (tid == 0) sq += epilogue<OP>(r0, s, ep);
  }
  if constexpr (NORM) {
    const double t = block_sum<kThreads>(sq, red);
    if (tid == 0) ep.partial[b] = t;
  }
}

// slices per wave of the dictionary kernel (env MLAMG_DICT_SPW = 1, 2 or 4; for A/B runs)
static int dict_slices_per_wave() {
  static int v = [] {
    const char* e = std::getenv("MLAMG_DICT_SPW");
    const int k = e ? std::atoi(e) : 2;
    return (k == 1 || k == 2 || k == 4) ? k : 2;
  }();
  return v;
}

// 256-pair chunks per workgroup of the row-pair kernel (measured: 2-4 best, 1 and 8 slower)
constexpr int kRpChunks = 4;

template <int OP, bool NORM, int CH, int K>
static int launch_rowpair_ck(const mlamg_csr* A, const double* x, const Epi& ep, hipStream_t s) {
  const int64_t n_pairs = (A->n_rows + 1) / 2;
  const unsigned nb = (unsigned)((n_pairs + CH * kThreads - 1) / (CH * kThreads));
  const size_t lds = (size_t)A->rp_n_ent * 32 + (size_t)A->rp_n_pat * 16 + 257 * 4;
  MLAMG_LAUNCH((k_rowpair<OP, NORM, CH, K>), dim3(nb), dim3(kThreads), lds, s, A->rp_pid,
                     A->rp_ptr, reinterpret_cast<const int4*>(A->rp_off),
                     reinterpret_cast<const dbl2*>(A->rp_val), A->rp_n_ent, A->n_rows,
                     A->n_cols, A->rp_dinv_att, reinterpret_cast<const dbl2*>(A->rp_dinv),
                     A->rp_n_pat, x, ep);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

template <int OP, bool NORM, int CH>
static int launch_rowpair_ch(const mlamg_csr* A, const double* x, const Epi& ep, hipStream_t s) {
  switch (A->rp_k) {  // the pattern step chosen at build time (longest pattern, 5..8)
    case 5: return launch_rowpair_ck<OP, NORM, CH, 5>(A, x, ep, s);
    case 6: return launch_rowpair_ck<OP, NORM, CH, 6>(A, x, ep, s);
    case 7: return launch_rowpair_ck<OP, NORM, CH, 7>(A, x, ep, s);
    default: return launch_rowpair_ck<OP, NORM, CH, 8>(A, x, ep, s);
  }
}

template <int OP, bool NORM, int CH>
static int launch_rowpat_uni(const mlamg_csr* A, const double* x, const Epi& ep, hipStream_t s) {
  const int64_t n_pairs = (A->n_rows + 1) / 2;
  const unsigned nb = (unsigned)((n_pairs + CH * kThreads - 1) / (CH * kThreads));
  const size_t lds = sizeof(dbl2) * (size_t)(CH * kThreads + A->rp_uni.halo + A->rp_n_pat) +
                     sizeof(uint16_t) * 256 + (size_t)A->rp_lds_pad;
#define MLAMG_RPU(LYV)                                                                           \
  MLAMG_LAUNCH((k_rowpat_uni<OP, NORM, CH, LYV>), dim3(nb), dim3(kThreads), lds, s,        \
                     A->rp_pid, A->rp_msk, A->rp_n_pat, A->n_rows, A->n_cols, A->rp_dinv_att,    \
                     reinterpret_cast<const dbl2*>(A->rp_dinv), A->rp_uni, x, ep)
  switch (A->rp_uni.layout) {
    case 1: MLAMG_RPU(1); break;
    case 2: MLAMG_RPU(2); break;
    case 3: MLAMG_RPU(3); break;
    case 4: MLAMG_RPU(4); break;
    default: MLAMG_RPU(0); break;
  }
#undef MLAMG_RPU
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

template <int OP, int CH, int PF>
static int launch_rowpat_march(const mlamg_csr* A, const double* x, const Epi& ep,
                               hipStream_t s) {
  constexpr int64_t T = 2 * CH * kThreads;
  const int64_t F = A->rp_mF;
  const int nt = (int)((F + T - 1) / T);
  const int64_t n_planes = (A->n_rows + F - 1) / F;
  const int seg = A->rp_mseg;
  const unsigned nb = (unsigned)(nt * ((n_planes + seg - 1) / seg));
  const size_t lds = sizeof(dbl2) * (size_t)(3 * (CH * kThreads + A->rp_uni.halo) + A->rp_n_pat) +
                     sizeof(uint16_t) * 256;
  MLAMG_LAUNCH((k_rowpat_march<OP, CH, PF>), dim3(nb), dim3(kThreads), lds, s, A->rp_pid, A->rp_msk,
               A->rp_n_pat, A->n_rows, A->rp_dinv_att, reinterpret_cast<const dbl2*>(A->rp_dinv),
               A->rp_uni, x, ep, F, nt, seg, n_planes);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

template <int OP, bool NORM>
static int launch_rowpair(const mlamg_csr* A, const double* x, const Epi& ep, hipStream_t s) {
  if constexpr (!NORM) {
    if (A->rp_mF > 0 && A->rp_msk)
      switch (A->rp_mch + 8 * A->rp_mpf) {
        case 1 + 8: return launch_rowpat_march<OP, 1, 1>(A, x, ep, s);
        case 2 + 8: return launch_rowpat_march<OP, 2, 1>(A, x, ep, s);
        case 4 + 8: return launch_rowpat_march<OP, 4, 1>(A, x, ep, s);
        case 1 + 16: return launch_rowpat_march<OP, 1, 2>(A, x, ep, s);
        default: return launch_rowpat_march<OP, 2, 2>(A, x, ep, s);
      }
  }
  if (rowpat_uniform(A)) {
    switch (A->rp_uni.ch) {
      case 1: return launch_rowpat_uni<OP, NORM, 1>(A, x, ep, s);
      case 2: return launch_rowpat_uni<OP, NORM, 2>(A, x, ep, s);
      default: return launch_rowpat_uni<OP, NORM, 4>(A, x, ep, s);
    }
  }
  if (A->rp_win.rows >= 0 && A->rp_slot) {
    const int64_t n_pairs = (A->n_rows + 1) / 2;
    const unsigned nb = (unsigned)((n_pairs + kRpWinNT - 1) / kRpWinNT);
    const size_t lds = sizeof(double) * (size_t)A->rp_win.rows;
#define MLAMG_RPW(KV)                                                                           \
  MLAMG_LAUNCH((k_rowpair_win<OP, NORM, KV>), dim3(nb), dim3(kRpWinNT), lds, s,            \
                     A->rp_slot, A->rp_ptr, reinterpret_cast<const int4*>(A->rp_off),           \
                     reinterpret_cast<const dbl2*>(A->rp_val), A->n_rows, A->n_cols,            \
                     A->rp_dinv_att, reinterpret_cast<const dbl2*>(A->rp_dinv), A->rp_win, x,   \
                     ep)
    switch (A->rp_k) {
      case 5: MLAMG_RPW(5); break;
      case 6: MLAMG_RPW(6); break;
      case 7: MLAMG_RPW(7); break;
      default: MLAMG_RPW(8); break;
    }
#undef MLAMG_RPW
    MLAMG_HIP(hipGetLastError());
    return MLAMG_OK;
  }
  return launch_rowpair_ch<OP, NORM, kRpChunks>(A, x, ep, s);
}

// ---------------------------------------------------------------- launch helpers
// MLAMG_NO_CACHED_LOADS=1: every nonzero stream non-temporal (A/B runs)
static bool cached_loads_off() {
  static const bool off = std::getenv("MLAMG_NO_CACHED_LOADS") != nullptr;
  return off;
}

template <int OP, bool NORM>
static int launch(const mlamg_csr* A, const double* x, const Epi& ep_in, hipStream_t s) {
  Epi ep = ep_in;
  ep.cached = A->n_rows == A->n_cols && A->nnz <= kCachedNnz && !cached_loads_off() ? 1 : 0;
  switch (active_format(A)) {
  case MLAMG_FMT_VECTOR:
    return launch_vec<OP, NORM>(A, x, ep, s);
  case MLAMG_FMT_LONG: {
    if (A->lg_nt == 0) return MLAMG_OK;
    MLAMG_LAUNCH((k_csr_long<OP, NORM>), dim3(A->lg_nt), dim3(kThreads), 0, s, A->indptr,
                       A->indices, A->data, A->lg_tile, x, ep);
    MLAMG_HIP(hipGetLastError());
    return MLAMG_OK;
  }
  case MLAMG_FMT_ROWPAT:
    if (A->n_rows == 0) return MLAMG_OK;
    return launch_rowpair<OP, NORM>(A, x, ep, s);
  case MLAMG_FMT_SORTED: {
    if (A->srt_nb == 0) return MLAMG_OK;
    const bool lr = A->avg_row_len >= kSrtLongRow;
#define MLAMG_SRT_LAUNCH(VMV, LRV)                                                              \
  MLAMG_LAUNCH((k_sorted<OP, NORM, VMV, LRV>), dim3(A->srt_nb), dim3(kSrtThreads), 0, s, \
                     A->indptr, A->srt_pk, A->srt_val, A->srt_vi, A->srt_vtab, A->srt_vc,      \
                     A->srt_vblk, A->srt_blk, A->srt_base, x, ep)
    if (A->srt_vi) {
      if (lr)
        MLAMG_SRT_LAUNCH(1, true);
      else
        MLAMG_SRT_LAUNCH(1, false);
    } else if (A->srt_vc) {
      if (lr)
        MLAMG_SRT_LAUNCH(2, true);
      else
        MLAMG_SRT_LAUNCH(2, false);
    } else {
      if (lr)
        MLAMG_SRT_LAUNCH(0, true);
      else
        MLAMG_SRT_LAUNCH(0, false);
    }
#undef MLAMG_SRT_LAUNCH
    MLAMG_HIP(hipGetLastError());
    return MLAMG_OK;
  }
  case MLAMG_FMT_SELL_DICT: {
    if (A->n_slices == 0) return MLAMG_OK;
    const int spw = dict_slices_per_wave();
    const int64_t per_block = (kThreads / 64) * spw;
    const unsigned nb = (unsigned)((A->n_slices + per_block - 1) / per_block);
    if (spw == 1)
      MLAMG_LAUNCH((k_sell_dict<OP, NORM, 1>), dim3(nb), dim3(kThreads), 0, s, A->dict_ptr,
                         A->dict_code, A->dict_off, A->dict_val, A->sell_perm, A->n_rows,
                         A->n_slices, x, ep);
    else if (spw == 2)
      MLAMG_LAUNCH((k_sell_dict<OP, NORM, 2>), dim3(nb), dim3(kThreads), 0, s, A->dict_ptr,
                         A->dict_code, A->dict_off, A->dict_val, A->sell_perm, A->n_rows,
                         A->n_slices, x, ep);
    else
      MLAMG_LAUNCH((k_sell_dict<OP, NORM, 4>), dim3(nb), dim3(kThreads), 0, s, A->dict_ptr,
                         A->dict_code, A->dict_off, A->dict_val, A->sell_perm, A->n_rows,
                         A->n_slices, x, ep);
    MLAMG_HIP(hipGetLastError());
    return MLAMG_OK;
  }
  case MLAMG_FMT_SELL: {
    if (A->n_slices == 0) return MLAMG_OK;
    const unsigned nb = (unsigned)((A->n_slices + kThreads / 64 - 1) / (kThreads / 64));
    MLAMG_LAUNCH((k_sell<OP, NORM>), dim3(nb), dim3(kThreads), 0, s, A->sell_ptr,
                       A->sell_col, A->sell_val, A->sell_perm, A->n_rows, A->n_slices, x, ep);
    MLAMG_HIP(hipGetLastError());
    return MLAMG_OK;
  }
  default:  // CSR-stream
    break;
  }
  if (A->n_blocks == 0) return MLAMG_OK;
  MLAMG_LAUNCH((k_csr_stream<OP, NORM>), dim3(A->n_blocks), dim3(kThreads), 0, s,
                     A->indptr, A->indices, A->data, A->blk, x, ep);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// The norm partials a NORM launch of A writes: the grid sizes of launch() and its helpers
int32_t norm_partials(const mlamg_csr* A) {
  const auto groups = [](int64_t n, int64_t per) {
    return (int32_t)std::max<int64_t>(1, (n + per - 1) / per);
  };
  switch (active_format(A)) {
    case MLAMG_FMT_VECTOR: return groups(A->n_rows, 1);  // one norm partial per row
    case MLAMG_FMT_LONG: return groups(A->lg_nt, 1);
    case MLAMG_FMT_ROWPAT:
      return groups((A->n_rows + 1) / 2,
                    rowpat_uniform(A)                       ? (int64_t)A->rp_uni.ch * kThreads
                    : (A->rp_win.rows >= 0 && A->rp_slot) ? (int64_t)kRpWinNT
                                                          : (int64_t)kRpChunks * kThreads);
    case MLAMG_FMT_SORTED: return A->srt_nb;
    case MLAMG_FMT_SELL_DICT: return groups(A->n_slices, (kThreads / 64) * dict_slices_per_wave());
    case MLAMG_FMT_SELL: return groups(A->n_slices, kThreads / 64);
    default: return A->n_blocks;
  }
}

int launch_spmv_plain(const mlamg_csr* A, const double* x, double* y, hipStream_t s) {
  Epi ep{};
  ep.alpha = 1.0;
  ep.beta = 0.0;
  ep.y = y;
  return launch<EPI_AXPBY, false>(A, x, ep, s);
}

// per-handle partial buffer for residual norms (slot 0 of the scratch cache is shared:
// callers on one stream only)
static double* partial_buf(const mlamg_csr* A) {
  return static_cast<double*>(scratch(sizeof(double) * part_capacity(A), 0));
}

int residual_impl(const mlamg_csr* A, const double* b, const double* x, double* r, double* norm2,
                  double* hist, int32_t* counter, int32_t* done, double tol, double* copy_to,
                  const double* copy_from, double* partial, hipStream_t s,
                  const double* smooth_dinv) {
  Epi ep{};
  ep.b = b;
  ep.y = r;
  ep.done = done;
  ep.copy_to = copy_to;
  ep.copy_from = copy_from;
  ep.dinv = copy_to ? smooth_dinv : nullptr;
  const bool want = norm2 || hist || counter;
  if (!want) return launch<EPI_RESID, false>(A, x, ep, s);
  ep.partial = partial ? partial : partial_buf(A);
  MLAMG_REQUIRE(ep.partial, "scratch allocation failed");
  MLAMG_TRY((launch<EPI_RESID, true>(A, x, ep, s)));
  hipLaunchKernelGGL(k_finalize_norm, dim3(1), dim3(1024), 0, s, ep.partial, A->n_part, norm2,
                     hist, counter, done, tol);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// r = b - A x with per-block sums of r^2 in partial[0..n_blocks) (no finalize), optional copy
int residual_partials(const mlamg_csr* A, const double* b, const double* x, double* r,
                      double* copy_to, const double* copy_from, double* partial,
                      const int32_t* done, hipStream_t s, const double* smooth_dinv) {
  Epi ep{};
  ep.b = b;
  ep.y = r;
  ep.done = done;
  ep.copy_to = copy_to;
  ep.copy_from = copy_from;
  ep.dinv = copy_to ? smooth_dinv : nullptr;
  ep.partial = partial;
  return launch<EPI_RESID, true>(A, x, ep, s);
}

int jacobi_sweep(const mlamg_csr* A, const double* dinv, const double* b, const double* xin,
                 double* xout, bool explicit_form, const int32_t* done, hipStream_t s) {
  Epi ep{};
  ep.b = b;
  ep.xin = xin;
  ep.dinv = dinv;
  ep.y = xout;
  ep.done = done;
  if (explicit_form) return launch<EPI_JACEXP, false>(A, xin, ep, s);
  return launch<EPI_JACOBI, false>(A, xin, ep, s);
}

int spmv_add(const mlamg_csr* A, const double* x, double* y, const int32_t* done, hipStream_t s) {
  Epi ep{};
  ep.y = y;
  ep.done = done;
  return launch<EPI_ADD, false>(A, x, ep, s);
}

// The polynomial smoother's launches (poly.hip). poly_first: r = b - A x (r nullable) and
// h = alpha * r, with xin set h = xin + alpha * r; h must not be x. poly_step: y = alpha * r + A h,
// with acc set y = xin + (alpha * r + A h), xin NULL standing for an all-zero one; y must not be h.
int poly_first(const mlamg_csr* A, const double* b, const double* x, double* r, double alpha,
               const double* xin, double* h, const int32_t* done, hipStream_t s) {
  Epi ep{};
  ep.alpha = alpha;
  ep.b = b;
  ep.y = r;
  ep.xin = xin;
  ep.copy_to = h;
  ep.done = done;
  return launch<EPI_POLY, false>(A, x, ep, s);
}

int poly_step(const mlamg_csr* A, double alpha, const double* r, const double* h, bool acc,
              const double* xin, double* y, const int32_t* done, hipStream_t s) {
  Epi ep{};
  ep.alpha = alpha;
  ep.beta = acc ? 1.0 : 0.0;
  ep.b = r;
  ep.xin = acc ? xin : nullptr;
  ep.y = y;
  ep.done = done;
  return launch<EPI_POLY, false>(A, h, ep, s);
}

// y += P e with P = (I - w D^-1 A) Agg applied factored (VERDICT r04 Next #5, opt-in): t = Agg e
// gathered into k_rowpat_uni's x window, y += t - (w / a_ii) (A t); dinv_w = w / a_ii (attached
// to A as its pattern table, else read per row). A in the uniform row-pair format only.
int spmv_fadd(const mlamg_csr* A, const int32_t* agg, const double* e, double* y,
              const double* dinv_w, const int32_t* done, hipStream_t s) {
  if (!rowpat_uniform(A) || A->n_rows != A->n_cols) {
    set_error("factored prolongation: the operator is not in the uniform row-pair format");
    return MLAMG_EUNSUPPORTED;
  }
  if (A->n_rows == 0) return MLAMG_OK;
  Epi ep{};
  ep.y = y;
  ep.dinv = dinv_w;
  ep.done = done;
  ep.agg = agg;
  switch (A->rp_uni.ch) {
    case 1: return launch_rowpat_uni<EPI_FADD, false, 1>(A, e, ep, s);
    case 2: return launch_rowpat_uni<EPI_FADD, false, 2>(A, e, ep, s);
    default: return launch_rowpat_uni<EPI_FADD, false, 4>(A, e, ep, s);
  }
}

int spmv_set(const mlamg_csr* A, const double* x, double* y, const int32_t* done, hipStream_t s,
             double* smooth_x, const double* smooth_dinv) {
  Epi ep{};
  ep.alpha = 1.0;
  ep.beta = 0.0;
  ep.y = y;
  ep.done = done;
  if (smooth_x) {
    ep.copy_to = smooth_x;  // smooth_x = smooth_dinv * y as well
    ep.dinv = smooth_dinv;
  }
  return launch<EPI_AXPBY, false>(A, x, ep, s);
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_spmv(const mlamg_csr* A, const double* x, double* y, double alpha, double beta,
               void* stream) {
  MLAMG_REQUIRE(A && (A->n_rows == 0 || (x && y)), "NULL argument");
  Epi ep{};
  ep.alpha = alpha;
  ep.beta = beta;
  ep.y = y;
  return launch<EPI_AXPBY, false>(A, x, ep, S(stream));
}

int mlamg_residual(const mlamg_csr* A, const double* b, const double* x, double* r, double* norm2,
                   void* stream) {
  MLAMG_REQUIRE(A && (A->n_rows == 0 || (b && x && r)), "NULL argument");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "residual needs a square matrix");
  return residual_impl(A, b, x, r, norm2, nullptr, nullptr, nullptr, kNoTol, nullptr, nullptr,
                       nullptr, S(stream));
}

int mlamg_jacobi(const mlamg_csr* A, const double* dinv_w, const double* b, double* x,
                 double* x_tmp, int nu, void* stream) {
  MLAMG_REQUIRE(A && (A->n_rows == 0 || (dinv_w && b && x && x_tmp)), "NULL argument");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "jacobi needs a square matrix");
  MLAMG_REQUIRE(nu >= 0, "nu < 0");
  MLAMG_REQUIRE(x != x_tmp, "x_tmp must differ from x");
  hipStream_t s = S(stream);
  double* cur = x;
  double* nxt = x_tmp;
  for (int i = 0; i < nu; ++i) {
    MLAMG_TRY(jacobi_sweep(A, dinv_w, b, cur, nxt, false, nullptr, s));
    std::swap(cur, nxt);
  }
  if (cur != x)
    MLAMG_HIP(hipMemcpyAsync(x, cur, sizeof(double) * A->n_rows, hipMemcpyDeviceToDevice, s));
  return MLAMG_OK;
}

int mlamg_jacobi_explicit(const mlamg_csr* M, const double* dinv_w, const double* b, double* x,
                          double* x_tmp, int nu, void* stream) {
  MLAMG_REQUIRE(M && (M->n_rows == 0 || (dinv_w && b && x && x_tmp)), "NULL argument");
  MLAMG_REQUIRE(M->n_rows == M->n_cols, "jacobi needs a square matrix");
  MLAMG_REQUIRE(nu >= 0, "nu < 0");
  MLAMG_REQUIRE(x != x_tmp, "x_tmp must differ from x");
  hipStream_t s = S(stream);
  double* cur = x;
  double* nxt = x_tmp;
  for (int i = 0; i < nu; ++i) {
    MLAMG_TRY(jacobi_sweep(M, dinv_w, b, cur, nxt, true, nullptr, s));
    std::swap(cur, nxt);
  }
  if (cur != x)
    MLAMG_HIP(hipMemcpyAsync(x, cur, sizeof(double) * M->n_rows, hipMemcpyDeviceToDevice, s));
  return MLAMG_OK;
}

int mlamg_restrict(const mlamg_csr* R, const double* r, double* r_c, void* stream) {
  MLAMG_REQUIRE(R && (R->n_rows == 0 || (r && r_c)), "NULL argument");
  return spmv_set(R, r, r_c, nullptr, S(stream));
}

int mlamg_prolong_add(const mlamg_csr* P, const double* e_c, double* x, void* stream) {
  MLAMG_REQUIRE(P && (P->n_rows == 0 || (e_c && x)), "NULL argument");
  return spmv_add(P, e_c, x, nullptr, S(stream));
}

}  // extern "C"
