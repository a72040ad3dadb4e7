// Block-diagonal dense coarse solve (include/mlamg.h mlamg_blockdense): the coarse operator of a
// batch of independent problems (mlamg/loss.py AmgLossBatch) is block diagonal, nb small blocks on
// the diagonal. Every block is inverted densely, all blocks in a handful of launches whatever nb
// is, and X = A_c^-1 B is one launch.
//
// Parity: block b's inverse is bitwise what mlamg_dense_create (dense.hip) builds for that block
// alone, and its rows of a solve are bitwise mlamg_dense_solve_mv on that block. The method per
// block follows dense.hip's rule: a block of >= 64 rows first tries the inverse Cholesky factor
// (dense_chol_inverse_batch: the bodies of the single call, many jobs per launch); a smaller block,
// and one that fails the symmetry or pivot test, takes Gauss-Jordan with partial pivoting. Blocks
// at or above dense_tri_min() rows (the single call keeps the factor there, method 2) are refused.
//
// The batched Gauss-Jordan (k_bd_gj_lds / k_bd_gj_global): one workgroup per block runs all n pivot
// steps in one launch, with the arithmetic of k_gj_row, k_eliminate and k_unpivot_cols (dense.hip)
// per element: the pivot of step k is the first argmax of |M[i][k]| over i >= k, row k is scaled by
// 1 / pivot (pivot slot <- 1 / pivot), M[i][j] - f * M[k][j] is a separate multiply and subtract,
// M[i][k] = -f * M[k][k], rows with f == 0.0 are skipped, and the interchanges are undone as column
// swaps last to first. Every element sees the same operations on the same operands in the same
// order as in the per-column launches of the single call; only the launch structure differs. The
// block lives in LDS when it fits (tiers of 16, 32, 64 and 128 rows: 128 x 128 doubles with the
// pivot column and the pivot indices are 130 of the CU's 160 KiB) and in its own slice of the
// handle's inverse buffer otherwise.
#include "common.hpp"
#include "reduce.hpp"

#include <memory>

struct mlamg_blockdense {
  int64_t nb = 0, n = 0;
  std::vector<int64_t> off;  // nb + 1 row offsets (host)
  std::vector<int> method;   // per block: mlamg_dense_info's method (0 or 1)
  double* inv = nullptr;     // the blocks' inverses, block b row-major n_b x n_b at invoff[b]
  int64_t* meta = nullptr;   // device: off (nb + 1) | invoff (nb + 1) | moff (nb + 1)
  int32_t* rowblk = nullptr; // device: the block of every stacked row
};

namespace mlamg {

namespace {

// rowblk[i] = b for the rows of block b (grid.y = block)
__global__ __launch_bounds__(256) void k_bd_rowblk(const int64_t* __restrict__ off,
                                                   int32_t* __restrict__ rowblk) {
  const int b = blockIdx.y;
  const int64_t i = off[b] + blockIdx.x * 256ll + threadIdx.x;
  if (i < off[b + 1]) rowblk[i] = b;
}

// k_densify per block: row i of the stacked CSR into its block of inv (and of the Cholesky work
// copy M where moff[b] >= 0); an entry outside the diagonal block is not written and its row is
// recorded (the smallest one) in *bad
__global__ __launch_bounds__(256) void k_bd_densify(const int32_t* __restrict__ ip,
                                                    const int32_t* __restrict__ ij,
                                                    const double* __restrict__ ax, int64_t n,
                                                    int64_t nb, const int64_t* __restrict__ meta,
                                                    const int32_t* __restrict__ rowblk,
                                                    double* __restrict__ inv,
                                                    double* __restrict__ M,
                                                    int32_t* __restrict__ bad) {
  const int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int b = rowblk[i];
  const int64_t o = meta[b], m = meta[b + 1] - o;
  const int64_t io = meta[nb + 1 + b], mo = meta[2 * (nb + 1) + b];
  double* r = inv + io + (i - o) * m;
  double* r2 = mo >= 0 ? M + mo + (i - o) * m : nullptr;
  for (int e = ip[i]; e < ip[i + 1]; ++e) {
    const int64_t c = (int64_t)ij[e] - o;
    if (c < 0 || c >= m) {
      atomicMin(bad, (int32_t)i);
      continue;
    }
    r[c] += ax[e];
    if (r2) r2[c] += ax[e];
  }
}

// Gauss-Jordan with partial pivoting of the n x n row-major M (leading dimension n), in place, by
// one workgroup of NT threads: dense.hip's k_gj_row + k_eliminate per pivot column, then
// k_unpivot_cols. colk: n doubles, piv: n int32 (LDS or global), wv / wi: NT / 64 slots of LDS.
// Returns false (in every thread) for an exactly singular M.
template <int NT>
__device__ __forceinline__ bool gj_invert(double* M, int n, double* colk, int32_t* piv, double* wv,
                                          int32_t* wi) {
  const int tid = threadIdx.x;
  for (int k = 0; k < n; ++k) {
    double best = -1.0;
    int32_t bidx = INT32_MAX;
    for (int i = k + tid; i < n; i += NT) {
      const double v = fabs(M[(int64_t)i * n + k]);
      if (v > best) {
        best = v;
        bidx = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o, 64);
      const int32_t oi = __shfl_xor(bidx, o, 64);
      if (ov > best || (ov == best && oi < bidx)) {
        best = ov;
        bidx = oi;
      }
    }
    if ((tid & 63) == 0) {
      wv[tid >> 6] = best;
      wi[tid >> 6] = bidx;
    }
    __syncthreads();
    best = wv[0];
    bidx = wi[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) {
      const double ov = wv[w];
      const int32_t oi = wi[w];
      if (ov > best || (ov == best && oi < bidx)) {
        best = ov;
        bidx = oi;
      }
    }
    const int32_t p = best > 0.0 ? bidx : -1;
    if (p < 0) return false;
    if (tid == 0) piv[k] = p;
    double* rk = M + (int64_t)k * n;
    if (p != k) {
      double* rp = M + (int64_t)p * n;
      for (int j = tid; j < n; j += NT) {
        const double t = rk[j];
        rk[j] = rp[j];
        rp[j] = t;
      }
    }
    __syncthreads();
    const double inv = 1.0 / rk[k];
    for (int j = tid; j < n; j += NT) colk[j] = M[(int64_t)j * n + k];
    __syncthreads();
    for (int j = tid; j < n; j += NT) rk[j] = (j == k) ? inv : rk[j] * inv;
    __syncthreads();
    // eliminate column k from every other row
    for (int i = tid / n, j = tid - (tid / n) * n; i < n;) {
      if (i != k) {
        const double f = colk[i];
        if (f != 0.0) {
          double* ri = M + (int64_t)i * n;
          ri[j] = (j == k) ? -f * rk[k] : ri[j] - f * rk[j];
        }
      }
      // advance (i, j) by NT elements without a division per element
      j += NT % n;
      i += NT / n;
      if (j >= n) {
        j -= n;
        ++i;
      }
    }
    __syncthreads();
  }
  // undo the row interchanges as column interchanges, last to first, a row per thread
  for (int i = tid; i < n; i += NT) {
    double* r = M + (int64_t)i * n;
    for (int k = n - 1; k >= 0; --k) {
      const int q = piv[k];
      if (q != k) {
        const double t = r[k];
        r[k] = r[q];
        r[q] = t;
      }
    }
  }
  __syncthreads();
  return true;
}

// blocks of at most CAP rows, held in LDS: workgroup w inverts block ids[w]
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void k_bd_gj_lds(const int32_t* __restrict__ ids, int64_t nb,
                                                  const int64_t* __restrict__ meta,
                                                  double* __restrict__ inv,
                                                  int32_t* __restrict__ fail) {
  __shared__ double sm[CAP * CAP];
  __shared__ double colk[CAP];
  __shared__ int32_t piv[CAP];
  __shared__ double wv[NT / 64];
  __shared__ int32_t wi[NT / 64];
  const int b = ids[blockIdx.x];
  const int n = (int)(meta[b + 1] - meta[b]);
  if (n <= 0 || n > CAP) return;
  double* G = inv + meta[nb + 1 + b];
  for (int q = threadIdx.x; q < n * n; q += NT) sm[q] = G[q];
  __syncthreads();
  if (!gj_invert<NT>(sm, n, colk, piv, wv, wi)) {
    if (threadIdx.x == 0) fail[b] = 1;
    return;
  }
  for (int q = threadIdx.x; q < n * n; q += NT) G[q] = sm[q];
}

// larger blocks, in place in the handle's buffer; colk / piv: the block's rows of two stacked
// work vectors
__global__ __launch_bounds__(1024) void k_bd_gj_global(const int32_t* __restrict__ ids, int64_t nb,
                                                       const int64_t* __restrict__ meta,
                                                       double* inv, double* colk, int32_t* piv,
                                                       int32_t* __restrict__ fail) {
  __shared__ double wv[16];
  __shared__ int32_t wi[16];
  const int b = ids[blockIdx.x];
  const int64_t o = meta[b];
  const int n = (int)(meta[b + 1] - o);
  if (n <= 0) return;
  if (!gj_invert<1024>(inv + meta[nb + 1 + b], n, colk + o, piv + o, wv, wi)) {
    if (threadIdx.x == 0) fail[b] = 1;
  }
}

// X_b = inv_b B_b: k_gemv_mv MODE 0 (spmm.hip) with the row's block in place of the one operator:
// a wave per row of the stacked coarse space, its block's row in lane-strided batches of 8
// (past-the-end slots add 0 * 0), the xor butterfly per column, the columns 8 at a time
constexpr int kBdCT = 8;
__global__ __launch_bounds__(256) void k_bd_gemv_mv(const double* __restrict__ inv, int64_t n,
                                                    int64_t nb, const int64_t* __restrict__ meta,
                                                    const int32_t* __restrict__ rowblk,
                                                    const double* __restrict__ B, int64_t ldb,
                                                    double* __restrict__ Xo, int64_t ldx, int k) {
  const int64_t row = blockIdx.x * 4ll + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const int b = rowblk[row];
  const int64_t o = meta[b], m = meta[b + 1] - o;
  const double* r = inv + meta[nb + 1 + b] + (row - o) * m;
  const double* Bb = B + o * ldb;
  for (int c0 = 0; c0 < k; c0 += kBdCT) {
    const int nc = min(kBdCT, k - c0);
    double s[kBdCT];
#pragma unroll
    for (int c = 0; c < kBdCT; ++c) s[c] = 0.0;
    for (int64_t j = lane; j < m; j += 8 * 64) {
      double mm[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t q = j + u * 64;
        mm[u] = q < m ? r[q] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t q = j + u * 64;
        const double* bp = Bb + q * ldb + c0;
#pragma unroll
        for (int c = 0; c < kBdCT; ++c) {
          const double v = (q < m && c < nc) ? bp[c] : 0.0;
          s[c] += mm[u] * v;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kBdCT; ++c) s[c] = wave_sum(s[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kBdCT; ++c)
        if (c < nc) Xo[row * ldx + c0 + c] = s[c];
    }
  }
}

void bd_free(mlamg_blockdense* D) {
  if (!D) return;
  if (D->inv) (void)hipFree(D->inv);
  if (D->meta) (void)hipFree(D->meta);
  if (D->rowblk) (void)hipFree(D->rowblk);
  delete D;
}

template <int CAP, int NT>
void launch_gj_tier(const std::vector<int32_t>& ids, const int32_t* d_ids, int64_t nb,
                    const int64_t* meta, double* inv, int32_t* fail, hipStream_t s) {
  if (ids.empty()) return;
  hipLaunchKernelGGL((k_bd_gj_lds<CAP, NT>), dim3((unsigned)ids.size()), dim3(NT), 0, s, d_ids, nb,
                     meta, inv, fail);
}

}  // namespace

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_blockdense_create(const mlamg_csr* A, const int64_t* offsets_host, int64_t nb,
                            mlamg_blockdense** out, void* stream) {
  MLAMG_REQUIRE(A, "A is NULL");
  MLAMG_REQUIRE(offsets_host, "offsets_host is NULL");
  MLAMG_REQUIRE(out, "out is NULL");
  MLAMG_REQUIRE(nb >= 1 && nb <= 65535, "nb must be in [1, 65535]");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "A: square matrix required");
  const int64_t n = A->n_rows;
  MLAMG_REQUIRE(offsets_host[0] == 0 && offsets_host[nb] == n,
                "offsets_host must run from 0 to the rows of A");
  const int64_t tri_min = dense_tri_min();
  int64_t max_n = 0, inv_total = 0, m_total = 0;
  const bool gj_only = std::getenv("MLAMG_DENSE_GJ") != nullptr;
  // host copy of the device table: off | invoff | moff (-1: no Cholesky work copy)
  std::vector<int64_t> meta(3 * (size_t)(nb + 1), -1);
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t m = offsets_host[b + 1] - offsets_host[b];
    MLAMG_REQUIRE(m >= 0, "offsets_host decreases at block " + std::to_string(b));
    MLAMG_REQUIRE(m < tri_min, "block " + std::to_string(b) + " has " + std::to_string(m) +
                                   " rows, at or above the factored dense solve's threshold of " +
                                   std::to_string(tri_min) +
                                   ": the batch is for small coarse problems (use "
                                   "mlamg_dense_create on that operator)");
    meta[b] = offsets_host[b];
    meta[nb + 1 + b] = inv_total;
    inv_total += m * m;
    if (m >= 64 && !gj_only) {
      meta[2 * (nb + 1) + b] = m_total;
      m_total += m * m;
    }
    max_n = std::max(max_n, m);
  }
  meta[nb] = n;
  meta[2 * nb + 1] = inv_total;
  hipStream_t s = S(stream);
  auto* D = new mlamg_blockdense();
  D->nb = nb;
  D->n = n;
  D->off.assign(offsets_host, offsets_host + nb + 1);
  D->method.assign((size_t)nb, 0);
  if (hipMalloc(&D->inv, sizeof(double) * std::max<int64_t>(inv_total, 1)) != hipSuccess ||
      hipMalloc(&D->meta, sizeof(int64_t) * meta.size()) != hipSuccess ||
      hipMalloc(&D->rowblk, sizeof(int32_t) * std::max<int64_t>(n, 1)) != hipSuccess) {
    bd_free(D);
    set_error("mlamg_blockdense_create: device allocation failed");
    return MLAMG_ENOMEM;
  }
  // work: Cholesky copies (slot 15); flags, block lists and the in-place variant's vectors (16)
  double* M = nullptr;
  if (m_total) {
    M = static_cast<double*>(scratch(sizeof(double) * (size_t)m_total, 15));
    if (!M) {
      bd_free(D);
      set_error("mlamg_blockdense_create: scratch allocation failed");
      return MLAMG_ENOMEM;
    }
  }
  // bad (1) | fail (nb) | ids (nb) int32, then colk (n doubles), piv (n int32)
  const size_t ints = ((size_t)(1 + 2 * nb) * sizeof(int32_t) + 255) & ~size_t(255);
  const size_t colk_b = ((size_t)std::max<int64_t>(n, 1) * sizeof(double) + 255) & ~size_t(255);
  char* w = static_cast<char*>(
      scratch(ints + colk_b + (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t), 16));
  if (!w) {
    bd_free(D);
    set_error("mlamg_blockdense_create: scratch allocation failed");
    return MLAMG_ENOMEM;
  }
  int32_t* bad = reinterpret_cast<int32_t*>(w);
  int32_t* fail = bad + 1;
  int32_t* d_ids = fail + nb;
  double* colk = reinterpret_cast<double*>(w + ints);
  int32_t* piv = reinterpret_cast<int32_t*>(w + ints + colk_b);
  auto fail_hip = [&](hipError_t e) {
    (void)hipStreamSynchronize(s);
    bd_free(D);
    set_error(std::string("mlamg_blockdense_create: ") + hipGetErrorString(e));
    return MLAMG_EHIP;
  };
  hipError_t e = hipMemcpyAsync(D->meta, meta.data(), sizeof(int64_t) * meta.size(),
                                hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(D->inv, 0, sizeof(double) * std::max<int64_t>(inv_total, 1), s);
  if (e == hipSuccess && m_total) e = hipMemsetAsync(M, 0, sizeof(double) * m_total, s);
  const int32_t int_max = INT32_MAX;
  if (e == hipSuccess) e = hipMemsetAsync(fail, 0, sizeof(int32_t) * nb, s);
  if (e == hipSuccess) e = hipMemcpyAsync(bad, &int_max, sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return fail_hip(e);
  if (n) {
    hipLaunchKernelGGL(k_bd_rowblk, dim3((unsigned)((max_n + 255) / 256), (unsigned)nb), dim3(256),
                       0, s, D->meta, D->rowblk);
    hipLaunchKernelGGL(k_bd_densify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A->indptr,
                       A->indices, A->data, n, nb, D->meta, D->rowblk, D->inv, M, bad);
  }
  // inverse Cholesky factor of every block of >= 64 rows (syncs)
  std::vector<DenseJob> jobs;
  std::vector<int64_t> job_block;
  for (int64_t b = 0; b < nb; ++b)
    if (meta[2 * (nb + 1) + b] >= 0) {
      DenseJob J{};
      J.M = M + meta[2 * (nb + 1) + b];
      J.inv = D->inv + meta[nb + 1 + b];
      J.n = meta[b + 1] - meta[b];
      jobs.push_back(J);
      job_block.push_back(b);
    }
  if (!jobs.empty()) {
    std::unique_ptr<bool[]> spd(new bool[jobs.size()]);
    const int rc = dense_chol_inverse_batch(jobs.data(), (int)jobs.size(), spd.get(), s);
    if (rc != MLAMG_OK) {
      (void)hipStreamSynchronize(s);
      bd_free(D);
      return rc;
    }
    for (size_t j = 0; j < jobs.size(); ++j)
      if (spd[j]) D->method[(size_t)job_block[j]] = 1;
  }
  // Gauss-Jordan of the others (their blocks of inv still hold the densified operator: the X^T X
  // product of a failed Cholesky job is not formed), a launch per size tier
  std::vector<int32_t> tier[5];
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t m = meta[b + 1] - meta[b];
    if (D->method[(size_t)b] != 0 || m == 0) continue;
    tier[m <= 16 ? 0 : m <= 32 ? 1 : m <= 64 ? 2 : m <= 128 ? 3 : 4].push_back((int32_t)b);
  }
  std::vector<int32_t> ids;
  size_t tier_at[5];
  for (int t = 0; t < 5; ++t) {
    tier_at[t] = ids.size();
    ids.insert(ids.end(), tier[t].begin(), tier[t].end());
  }
  if (!ids.empty()) {
    e = hipMemcpyAsync(d_ids, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail_hip(e);
    launch_gj_tier<16, 256>(tier[0], d_ids + tier_at[0], nb, D->meta, D->inv, fail, s);
    launch_gj_tier<32, 256>(tier[1], d_ids + tier_at[1], nb, D->meta, D->inv, fail, s);
    launch_gj_tier<64, 256>(tier[2], d_ids + tier_at[2], nb, D->meta, D->inv, fail, s);
    launch_gj_tier<128, 1024>(tier[3], d_ids + tier_at[3], nb, D->meta, D->inv, fail, s);
    if (!tier[4].empty())
      hipLaunchKernelGGL(k_bd_gj_global, dim3((unsigned)tier[4].size()), dim3(1024), 0, s,
                         d_ids + tier_at[4], nb, D->meta, D->inv, colk, piv, fail);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e);
  std::vector<int32_t> h((size_t)nb + 1);
  e = hipMemcpyAsync(h.data(), bad, sizeof(int32_t) * (nb + 1), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail_hip(e);
  if (h[0] != INT32_MAX) {
    bd_free(D);
    set_error("mlamg_blockdense_create: row " + std::to_string(h[0]) +
              " has an entry outside the diagonal blocks");
    return MLAMG_EINVAL;
  }
  for (int64_t b = 0; b < nb; ++b)
    if (h[(size_t)b + 1]) {
      bd_free(D);
      set_error("mlamg_blockdense_create: block " + std::to_string(b) + " is exactly singular");
      return MLAMG_EINVAL;
    }
  *out = D;
  return MLAMG_OK;
}

int mlamg_blockdense_info(const mlamg_blockdense* D, int64_t* nb, int64_t* n, int* methods) {
  MLAMG_REQUIRE(D, "D is NULL");
  if (nb) *nb = D->nb;
  if (n) *n = D->n;
  if (methods)
    for (int64_t b = 0; b < D->nb; ++b) methods[b] = D->method[(size_t)b];
  return MLAMG_OK;
}

int mlamg_blockdense_destroy(mlamg_blockdense* D) {
  bd_free(D);
  return MLAMG_OK;
}

int mlamg_blockdense_solve_mv(const mlamg_blockdense* D, const double* B, int64_t ldb, double* X,
                              int64_t ldx, int k, void* stream) {
  MLAMG_REQUIRE(D, "D is NULL");
  MLAMG_REQUIRE(B, "B is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldb >= k, "ldb < k");
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(B != X, "B and X must differ");
  if (D->n == 0) return MLAMG_OK;
  hipLaunchKernelGGL(k_bd_gemv_mv, dim3((unsigned)((D->n + 3) / 4)), dim3(256), 0, S(stream),
                     D->inv, D->n, D->nb, D->meta, D->rowblk, B, ldb, X, ldx, k);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

}  // extern "C"
