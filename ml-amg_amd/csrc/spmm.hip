// Multi-vector (n x k) kernels: SpMM with the V-cycle epilogues, per-column norms and mean
// removal, the dense coarse solve on a block (include/mlamg.h "multi-vector path").
//
// A multivector is fp64 row-major n x k with a leading dimension ld >= k. Every kernel keeps the
// arithmetic of its single-vector counterpart PER COLUMN: a row is summed left to right in stored
// order with separate multiply and add (scipy's csr_matvecs), the reductions keep the partition
// and order of k_sumsq_partial / k_sum_sqrt (vec.hip), k_ls_sum / k_ls_total (lsqr.hip) and k_gemv
// (dense.hip). Column j of every result is therefore bitwise the single-vector result on column j.
//
// k_spmm_stream has k_csr_stream's shape: one 256-thread workgroup per row block (<= 256 rows,
// <= 2048 nonzeros, or one over-long row) stages the block's column indices and values in LDS
// with coalesced non-temporal loads — the matrix stream is read once for all k columns — and then
// deals its (row, column pair) work items over the lanes: a lane owns two adjacent columns of one
// row (two accumulators in registers), neighbouring lanes own neighbouring column pairs of the same
// row, so one gather instruction of a wave reads 64/ceil(k/2) whole X rows as contiguous 16-byte
// pieces (k = 8: 64-byte runs, k >= 16: full 128-byte lines). The 16-byte accesses need 16-byte
// aligned pointers and even leading dimensions (VEC); otherwise the same kernel runs with 8-byte
// accesses.
#include "common.hpp"
#include "reduce.hpp"
#include "spmm_epi.hpp"

#include <hip/hip_runtime.h>

namespace mlamg {

__device__ __forceinline__ int64_t xcd_block_mv(int64_t b, int64_t nb) {
  const int64_t q = nb >> 3, r = nb & 7, g = b & 7, i = b >> 3;
  return (g < r ? g * (q + 1) : r * (q + 1) + (g - r) * q) + i;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_spmm_stream(const int32_t* __restrict__ indptr,
                                                          const int32_t* __restrict__ indices,
                                                          const double* __restrict__ vals,
                                                          const int32_t* __restrict__ blk,
                                                          const double* __restrict__ X,
                                                          int64_t ldx, int k, EpiMV ep) {
  __shared__ double sv[kBlockNnz];
  __shared__ int32_t sc[kBlockNnz];
  __shared__ int32_t rp[kBlockRows + 1];
  if (ep.done && *ep.done) return;
  const int b = (int)xcd_block_mv(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  const int r0 = blk[b];
  const int r1 = blk[b + 1];
  const int nr = r1 - r0;
  const int e0 = indptr[r0];
  const int ne = indptr[r1] - e0;
  const int nch = (k + 1) >> 1;  // column pairs
  if (ne <= kBlockNnz) {
    const int32_t* ci = indices + e0;
    const double* cv = vals + e0;
    constexpr int U = kBlockNnz / kThreads;
    int32_t cc[U];
    double vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = tid + u * kThreads;
      cc[u] = e < ne ? __builtin_nontemporal_load(ci + e) : 0;
      vv[u] = e < ne ? __builtin_nontemporal_load(cv + e) : 0.0;
    }
    for (int t = tid; t <= nr; t += kThreads) rp[t] = indptr[r0 + t] - e0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = tid + u * kThreads;
      if (e < ne) {
        sc[e] = cc[u];
        sv[e] = vv[u];
      }
    }
    __syncthreads();
    const int items = nr * nch;
    for (int w = tid; w < items; w += kThreads) {
      const int t = w / nch;
      const int c = (w - t * nch) << 1;
      const bool two = c + 1 < k;
      const double* xc = X + c;
      const int ka = rp[t], kb = rp[t + 1];
      double s0 = 0.0, s1 = 0.0;
      int e = ka;
      for (; e + 4 <= kb; e += 4) {
        double xa[4], xb[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v[u] = sv[e + u];
          ld2<VEC>(xc + (int64_t)sc[e + u] * ldx, two, xa[u], xb[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s0 += v[u] * xa[u];
          s1 += v[u] * xb[u];
        }
      }
      for (; e < kb; ++e) {
        double xa, xb;
        const double v = sv[e];
        ld2<VEC>(xc + (int64_t)sc[e] * ldx, two, xa, xb);
        s0 += v * xa;
        s1 += v * xb;
      }
      epi_mv<VEC>(r0 + t, c, two, s0, s1, ep);
    }
  } else {
    // one over-long row: stream it through LDS in chunks; lane p keeps the ordered sums of the
    // column pair (2p, 2p + 1) (nch <= 32 lanes)
    const int c = tid << 1;
    const bool mine = tid < nch;
    const bool two = c + 1 < k;
    double s0 = 0.0, s1 = 0.0;
    for (int c0 = 0; c0 < ne; c0 += kBlockNnz) {
      const int m = min(kBlockNnz, ne - c0);
      for (int e = tid; e < m; e += kThreads) {
        sc[e] = indices[e0 + c0 + e];
        sv[e] = vals[e0 + c0 + e];
      }
      __syncthreads();
      if (mine) {
        const double* xc = X + c;
        for (int e = 0; e < m; ++e) {
          double xa, xb;
          const double v = sv[e];
          ld2<VEC>(xc + (int64_t)sc[e] * ldx, two, xa, xb);
          s0 += v * xa;
          s1 += v * xb;
        }
      }
      __syncthreads();
    }
    if (mine) epi_mv<VEC>(r0, c, two, s0, s1, ep);
  }
}

// One SpMM launch with epilogue `ep` (pointers and leading dimensions already validated). canon:
// rows summed in the canonical CSR-vector order (spmm_vec.hip) instead of scipy's.
static int launch_spmm(const mlamg_csr* A, const double* X, int64_t ldx, int k, const EpiMV& ep,
                       hipStream_t s, bool canon) {
  if (canon) return launch_spmm_vcan(A, X, ldx, k, ep, s);
  if (A->n_rows == 0 || A->n_blocks == 0) return MLAMG_OK;
  MLAMG_REQUIRE(A->blk != nullptr, "operator has no row-block table");
  if (mv_vec16(X, ldx, ep)) {
    MLAMG_LAUNCH((k_spmm_stream<true>), dim3(A->n_blocks), dim3(kThreads), 0, s, A->indptr,
                 A->indices, A->data, A->blk, X, ldx, k, ep);
  } else {
    MLAMG_LAUNCH((k_spmm_stream<false>), dim3(A->n_blocks), dim3(kThreads), 0, s, A->indptr,
                 A->indices, A->data, A->blk, X, ldx, k, ep);
  }
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int spmm_set_mv(const mlamg_csr* A, const double* X, int64_t ldx, double* Y, int64_t ldy, int k,
                double alpha, double beta, hipStream_t s, const int32_t* done, bool canon) {
  EpiMV ep{};
  ep.done = done;
  ep.op = MV_AXPBY;
  ep.alpha = alpha;
  ep.beta = beta;
  ep.Y = Y;
  ep.ldy = ldy;
  return launch_spmm(A, X, ldx, k, ep, s, canon);
}

int spmm_add_mv(const mlamg_csr* A, const double* X, int64_t ldx, double* Y, int64_t ldy, int k,
                hipStream_t s, const int32_t* done, bool canon) {
  EpiMV ep{};
  ep.done = done;
  ep.op = MV_ADD;
  ep.Y = Y;
  ep.ldy = ldy;
  return launch_spmm(A, X, ldx, k, ep, s, canon);
}

int residual_mv(const mlamg_csr* A, const double* B, int64_t ldb, const double* X, int64_t ldx,
                double* R, int64_t ldr, int k, hipStream_t s, const int32_t* done, bool canon) {
  EpiMV ep{};
  ep.done = done;
  ep.op = MV_RESID;
  ep.B = B;
  ep.ldb = ldb;
  ep.Y = R;
  ep.ldy = ldr;
  return launch_spmm(A, X, ldx, k, ep, s, canon);
}

int jacobi_sweep_mv(const mlamg_csr* A, const double* dinv, const double* B, int64_t ldb,
                    const double* Xin, int64_t ldxin, double* Xout, int64_t ldxout, int k,
                    hipStream_t s, const int32_t* done, bool canon) {
  EpiMV ep{};
  ep.done = done;
  ep.op = MV_JACOBI;
  ep.B = B;
  ep.ldb = ldb;
  ep.Xin = Xin;
  ep.ldxin = ldxin;
  ep.dinv = dinv;
  ep.Y = Xout;
  ep.ldy = ldxout;
  return launch_spmm(A, Xin, ldxin, k, ep, s, canon);
}

// the polynomial smoother's launches on a block (spmv.hip poly_first / poly_step per column)
int poly_first_mv(const mlamg_csr* A, const double* B, int64_t ldb, const double* X, int64_t ldx,
                  double* R, int64_t ldr, double alpha, const double* Xin, int64_t ldxin, double* H,
                  int64_t ldh, int k, hipStream_t s, const int32_t* done, bool canon) {
  EpiMV ep{};
  ep.done = done;
  ep.op = MV_POLY;
  ep.alpha = alpha;
  ep.B = B;
  ep.ldb = ldb;
  ep.Xin = Xin;
  ep.ldxin = ldxin;
  ep.Y = R;
  ep.ldy = ldr;
  ep.H = H;
  ep.ldh = ldh;
  return launch_spmm(A, X, ldx, k, ep, s, canon);
}

int poly_step_mv(const mlamg_csr* A, double alpha, const double* R, int64_t ldr, const double* H,
                 int64_t ldh, bool acc, const double* Xin, int64_t ldxin, double* Y, int64_t ldy,
                 int k, hipStream_t s, const int32_t* done, bool canon) {
  EpiMV ep{};
  ep.done = done;
  ep.op = MV_POLY;
  ep.alpha = alpha;
  ep.beta = acc ? 1.0 : 0.0;
  ep.B = R;
  ep.ldb = ldr;
  ep.Xin = acc ? Xin : nullptr;
  ep.ldxin = ldxin;
  ep.Y = Y;
  ep.ldy = ldy;
  return launch_spmm(A, H, ldh, k, ep, s, canon);
}

// ---------------------------------------------------------------- row-wise vector kernels
// X[i, :] += d[i] * R[i, :] (mode 0: k_axpy_diag per column) or X[i, :] = d[i] * B[i, :] (mode 1:
// k_mul_diag per column); one element per thread, columns fastest
__global__ __launch_bounds__(256) void k_diag_mv(double* __restrict__ X, int64_t ldx,
                                                 const double* __restrict__ d,
                                                 const double* __restrict__ R, int64_t ldr,
                                                 int64_t n, int k, int mode,
                                                 const int32_t* __restrict__ done) {
  const int64_t w = blockIdx.x * 256ll + threadIdx.x;
  if (w >= n * k || (done && *done)) return;
  const int64_t i = w / k;
  const int c = (int)(w - i * k);
  const double r = R[i * ldr + c];
  if (mode == 0) {
    X[i * ldx + c] = X[i * ldx + c] + d[i] * r;
  } else {
    X[i * ldx + c] = d[i] * r;
  }
}

int diag_mv(double* X, int64_t ldx, const double* d, const double* R, int64_t ldr, int64_t n,
            int k, int mode, hipStream_t s, const int32_t* done) {
  if (n == 0) return MLAMG_OK;
  const int64_t nb = (n * k + 255) / 256;
  hipLaunchKernelGGL(k_diag_mv, dim3((unsigned)nb), dim3(256), 0, s, X, ldx, d, R, ldr, n, k, mode,
                     done);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// ---------------------------------------------------------------- per-column norms
// k_sumsq_partial (SQ) / k_ls_sum (!SQ) on the columns [8 blockIdx.y, 8 blockIdx.y + 8): thread t
// of block b walks the rows b*256 + t + m*gridDim.x*256 exactly as the single-vector kernel
// does, with one accumulator per column; partial[col * gridDim.x + b]
template <bool SQ>
__global__ __launch_bounds__(256) void k_colsum_partial(const double* __restrict__ X, int64_t ldx,
                                                        int64_t n, int k,
                                                        double* __restrict__ partial) {
  __shared__ double red[4][kColTile];
  const int c0 = blockIdx.y * kColTile;
  const int nc = min(kColTile, k - c0);
  double acc[kColTile];
#pragma unroll
  for (int c = 0; c < kColTile; ++c) acc[c] = 0.0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double* p = X + i * ldx + c0;
#pragma unroll
    for (int c = 0; c < kColTile; ++c) {
      if (c < nc) {
        const double v = p[c];
        if constexpr (SQ) {
          acc[c] += v * v;
        } else {
          acc[c] += v;
        }
      }
    }
  }
  const bool mine = (int)threadIdx.x < nc;
  const double t = tile_sum<256>(acc, red, mine);
  if (mine) partial[(int64_t)(c0 + threadIdx.x) * gridDim.x + blockIdx.x] = t;
}

// k_sum_sqrt per column: block j sums column j's nb partials and writes sqrt to out[j]
__global__ __launch_bounds__(1024) void k_colsum_sqrt(const double* __restrict__ partial, int nb,
                                                      double* __restrict__ out) {
  __shared__ double red[16];
  const double* p = partial + (int64_t)blockIdx.x * nb;
  const double t = partials_total<1024>(p, nb, red);
  if (threadIdx.x == 0) out[blockIdx.x] = sqrt(t);
}

int norm2_mv(const double* X, int64_t ldx, int64_t n, int k, double* out, hipStream_t s) {
  double* partial =
      static_cast<double*>(scratch(sizeof(double) * kNormGridCap * MLAMG_MV_MAX, 8));
  MLAMG_REQUIRE(partial, "scratch allocation failed");
  const int nb = reduce_grid(n, 256, kNormGridCap);
  hipLaunchKernelGGL(k_colsum_partial<true>, dim3(nb, (k + kColTile - 1) / kColTile), dim3(256), 0, s, X,
                     ldx, n, k, partial);
  hipLaunchKernelGGL(k_colsum_sqrt, dim3(k), dim3(1024), 0, s, partial, nb, out);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// ---------------------------------------------------------------- per-column mean removal
// k_ls_total per column (256 threads over the 512 partials of column blockIdx.x)
__global__ __launch_bounds__(256) void k_coltotal(const double* __restrict__ partial,
                                                  double* __restrict__ out) {
  __shared__ double red[4];
  const double* p = partial + (int64_t)blockIdx.x * kSumGrid;
  const double t = partials_total<256>(p, kSumGrid, red);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// k_ls_sub_mean per column
__global__ __launch_bounds__(256) void k_colsub_mean(double* __restrict__ X, int64_t ldx, int64_t n,
                                                     int k, const double* __restrict__ sum) {
  const int64_t w = blockIdx.x * 256ll + threadIdx.x;
  if (w >= n * k) return;
  const int64_t i = w / k;
  const int c = (int)(w - i * k);
  const double mean = sum[c] / (double)n;
  X[i * ldx + c] = X[i * ldx + c] - mean;
}

int remove_mean_mv(double* X, int64_t ldx, int64_t n, int k, hipStream_t s) {
  if (n == 0) return MLAMG_OK;
  double* partial = static_cast<double*>(
      scratch(sizeof(double) * (kSumGrid + 1) * MLAMG_MV_MAX, 9));
  MLAMG_REQUIRE(partial, "scratch allocation failed");
  double* total = partial + (int64_t)kSumGrid * MLAMG_MV_MAX;
  hipLaunchKernelGGL(k_colsum_partial<false>, dim3(kSumGrid, (k + kColTile - 1) / kColTile),
                     dim3(256), 0, s, X, ldx, n, k, partial);
  hipLaunchKernelGGL(k_coltotal, dim3(k), dim3(256), 0, s, partial, total);
  hipLaunchKernelGGL(k_colsub_mean, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, s, X, ldx,
                     n, k, total);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// ---------------------------------------------------------------- dense coarse solve on a block
// k_gemv / k_gemv_tri (dense.hip) with one accumulator per column: a wave per row of M, the same
// lane-strided batches of 8 (past-the-end slots add 0 * 0) and xor butterfly per column; the
// columns are taken 8 at a time, the row of M staying in cache between tiles.
// MODE 0: all of the row; 1: columns [0, row] (y = X b); 2: columns [row, n) (x = X^T y)
template <int MODE>
__global__ __launch_bounds__(256) void k_gemv_mv(const double* __restrict__ M, int64_t n,
                                                 const double* __restrict__ B, int64_t ldb,
                                                 double* __restrict__ Xo, int64_t ldx, int k,
                                                 const int32_t* __restrict__ done) {
  const int64_t row = blockIdx.x * 4ll + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n || (done && *done)) return;
  const double* r = M + row * n;
  const int64_t j0 = MODE == 2 ? row : 0, j1 = MODE == 1 ? row + 1 : n;
  for (int c0 = 0; c0 < k; c0 += kColTile) {
    const int nc = min(kColTile, k - c0);
    double s[kColTile];
#pragma unroll
    for (int c = 0; c < kColTile; ++c) s[c] = 0.0;
    for (int64_t j = j0 + lane; j < j1; j += 8 * 64) {
      double m[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t q = j + u * 64;
        m[u] = q < j1 ? r[q] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t q = j + u * 64;
        const double* bp = B + q * ldb + c0;
#pragma unroll
        for (int c = 0; c < kColTile; ++c) {
          const double v = (q < j1 && c < nc) ? bp[c] : 0.0;
          s[c] += m[u] * v;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kColTile; ++c) {
      s[c] = wave_sum(s[c]);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kColTile; ++c)
        if (c < nc) Xo[row * ldx + c0 + c] = s[c];
    }
  }
}

// X = A_c^-1 B; ytmp: n x k scratch (leading dimension k) of method 2's intermediate X b
int dense_solve_mv(const mlamg_dense* D, const double* B, int64_t ldb, double* X, int64_t ldx,
                   int k, double* ytmp, hipStream_t s, const int32_t* done) {
  if (D->n == 0) return MLAMG_OK;
  const dim3 g((unsigned)((D->n + 3) / 4));
  if (D->method == 2) {
    MLAMG_REQUIRE(ytmp, "scratch allocation failed");
    hipLaunchKernelGGL(k_gemv_mv<1>, g, dim3(256), 0, s, D->inv, D->n, B, ldb, ytmp, (int64_t)k, k,
                       done);
    hipLaunchKernelGGL(k_gemv_mv<2>, g, dim3(256), 0, s, D->inv, D->n, ytmp, (int64_t)k, X, ldx, k,
                       done);
  } else {
    hipLaunchKernelGGL(k_gemv_mv<0>, g, dim3(256), 0, s, D->inv, D->n, B, ldb, X, ldx, k, done);
  }
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// ---------------------------------------------------------------- bodies of the twin C entries
// What mlamg_residual_mv / mlamg_jacobi_mv and their _vec twins (spmm_vec.hip) do once each has
// checked its arguments; canon picks the summation order.
int residual_mv_run(const mlamg_csr* A, const double* B, int64_t ldb, const double* X, int64_t ldx,
                    double* R, int64_t ldr, int k, double* norms, hipStream_t s, bool canon) {
  MLAMG_TRY(residual_mv(A, B, ldb, X, ldx, R, ldr, k, s, nullptr, canon));
  if (norms) MLAMG_TRY(norm2_mv(R, ldr, A->n_rows, k, norms, s));
  return MLAMG_OK;
}

// nu sweeps ping-ponging between X and X_tmp; the result is copied back when it ends in X_tmp
int jacobi_mv_run(const mlamg_csr* A, const double* dinv_w, const double* B, int64_t ldb, double* X,
                  int64_t ldx, double* X_tmp, int64_t ldt, int k, int nu, hipStream_t s,
                  bool canon) {
  double* cur = X;
  double* nxt = X_tmp;
  int64_t lc = ldx, ln = ldt;
  for (int i = 0; i < nu; ++i) {
    MLAMG_TRY(jacobi_sweep_mv(A, dinv_w, B, ldb, cur, lc, nxt, ln, k, s, nullptr, canon));
    std::swap(cur, nxt);
    std::swap(lc, ln);
  }
  if (cur != X && A->n_rows > 0)
    MLAMG_HIP(hipMemcpy2DAsync(X, sizeof(double) * ldx, cur, sizeof(double) * lc,
                               sizeof(double) * k, A->n_rows, hipMemcpyDeviceToDevice, s));
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_spmm(const mlamg_csr* A, const double* X, int64_t ldx, double* Y, int64_t ldy, int k,
               double alpha, double beta, void* stream) {
  MLAMG_REQUIRE(A && X && Y, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k && ldy >= k, "leading dimension < k");
  MLAMG_REQUIRE(X != Y, "X and Y must differ");
  return spmm_set_mv(A, X, ldx, Y, ldy, k, alpha, beta, S(stream));
}

int mlamg_residual_mv(const mlamg_csr* A, const double* B, int64_t ldb, const double* X,
                      int64_t ldx, double* R, int64_t ldr, int k, double* norms, void* stream) {
  MLAMG_REQUIRE(A && X && R, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k && ldr >= k && (!B || ldb >= k), "leading dimension < k");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "residual needs a square matrix");
  MLAMG_REQUIRE(X != R, "X and R must differ");
  return residual_mv_run(A, B, ldb, X, ldx, R, ldr, k, norms, S(stream), false);
}

int mlamg_jacobi_mv(const mlamg_csr* A, const double* dinv_w, const double* B, int64_t ldb,
                    double* X, int64_t ldx, double* X_tmp, int64_t ldt, int k, int nu,
                    void* stream) {
  MLAMG_REQUIRE(A && dinv_w && X && X_tmp, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k && ldt >= k && (!B || ldb >= k), "leading dimension < k");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "jacobi needs a square matrix");
  MLAMG_REQUIRE(nu >= 0, "nu < 0");
  MLAMG_REQUIRE(X != X_tmp, "X_tmp must differ from X");
  return jacobi_mv_run(A, dinv_w, B, ldb, X, ldx, X_tmp, ldt, k, nu, S(stream), false);
}

int mlamg_restrict_mv(const mlamg_csr* R, const double* Rf, int64_t ldr, double* Bc, int64_t ldb,
                      int k, void* stream) {
  MLAMG_REQUIRE(R && Rf && Bc, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldr >= k && ldb >= k, "leading dimension < k");
  return spmm_set_mv(R, Rf, ldr, Bc, ldb, k, 1.0, 0.0, S(stream));
}

int mlamg_prolong_add_mv(const mlamg_csr* P, const double* E, int64_t lde, double* X, int64_t ldx,
                         int k, void* stream) {
  MLAMG_REQUIRE(P && E && X, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(lde >= k && ldx >= k, "leading dimension < k");
  return spmm_add_mv(P, E, lde, X, ldx, k, S(stream));
}

int mlamg_norm2_mv(const double* X, int64_t ldx, int64_t n, int k, double* out, void* stream) {
  MLAMG_REQUIRE(out && (n == 0 || X), "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "leading dimension < k");
  MLAMG_REQUIRE(n >= 0, "n < 0");
  return norm2_mv(X, ldx, n, k, out, S(stream));
}

int mlamg_remove_mean_mv(double* X, int64_t ldx, int64_t n, int k, void* stream) {
  MLAMG_REQUIRE(n >= 0 && (n == 0 || X), "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "leading dimension < k");
  return remove_mean_mv(X, ldx, n, k, S(stream));
}

int mlamg_dense_solve_mv(const mlamg_dense* D, const double* B, int64_t ldb, double* X,
                         int64_t ldx, int k, void* stream) {
  MLAMG_REQUIRE(D && B && X, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldb >= k && ldx >= k, "leading dimension < k");
  MLAMG_REQUIRE(B != X, "B and X must differ");
  double* ytmp = nullptr;
  if (D->method == 2)
    ytmp = static_cast<double*>(scratch(sizeof(double) * (size_t)D->n * (size_t)k, 10));
  return dense_solve_mv(D, B, ldb, X, ldx, k, ytmp, S(stream));
}

}  // extern "C"
