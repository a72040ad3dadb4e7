// lambda_max(D^-1 A) for the smoothed-aggregation weight omega = (4/3)/lambda_max
// (ns/lib/multigrid.py:105: ARPACK eigs(Dinv@A, k=1, which='LM')).
//
// D^-1 A is self-adjoint in the D inner product <x, y>_D = x^T D y (A symmetric, positive
// diagonal), so Lanczos in that inner product converges to its extreme eigenvalue with plain
// products by A: q_j D-orthonormal, z = A q_j, alpha_j = z . q_j,
// w = D^-1 z - alpha_j q_j - beta_j q_{j-1}, beta_{j+1} = ||w||_D, q_{j+1} = w / beta_{j+1}.
// The product z = A q is the operator's own SpMV kernel in whatever format it carries (the C4
// fine level in the row-pair format: 37 us instead of 250 us for a CSR pass with the scaling
// fused), the vector work is three streaming kernels and the three Lanczos vectors rotate by
// pointer. alpha_j and beta_j stay on the device; the host reads them every kCheck iterations
// to bisect the tridiagonal T_j for its largest eigenvalue. Reductions use a fixed order, so
// the result is deterministic.
#include "common.hpp"
#include "reduce.hpp"
#include "tridiag.hpp"

#include <cmath>

namespace mlamg {

__global__ __launch_bounds__(1024) void k_reduce_to(const double* __restrict__ partial, int n,
                                                    double* __restrict__ out, int take_sqrt) {
  __shared__ double red[16];
  const double t = partials_total<1024>(partial, n, red);
  if (threadIdx.x == 0) *out = take_sqrt ? sqrt(t) : t;
}

// partial[b] = sum over the block's entries of z_i q_i
__global__ __launch_bounds__(256) void k_lz_dot(const double* __restrict__ z,
                                                const double* __restrict__ q, int64_t n,
                                                double* __restrict__ partial) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    acc += z[i] * q[i];
  const double t = block_sum_all<256>(acc, red);
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// w = D^-1 z - alpha q - beta q_prev ; partial = sum d_i w_i^2 (the D-norm)
__global__ __launch_bounds__(256) void k_lz_update(const double* __restrict__ z,
                                                   const double* __restrict__ dinv,
                                                   const double* __restrict__ d,
                                                   const double* __restrict__ q,
                                                   const double* __restrict__ qprev,
                                                   const double* __restrict__ alpha,
                                                   const double* __restrict__ beta, int64_t n,
                                                   double* __restrict__ w,
                                                   double* __restrict__ partial) {
  __shared__ double red[4];
  const double a = *alpha, bt = *beta;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double wi = (dinv[i] * z[i] - a * q[i]) - bt * qprev[i];
    w[i] = wi;
    acc += d[i] * (wi * wi);
  }
  const double t = block_sum_all<256>(acc, red);
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// w <- w / beta (beta = 0: breakdown, w = 0)
__global__ __launch_bounds__(256) void k_lz_scale(double* __restrict__ w,
                                                  const double* __restrict__ beta, int64_t n) {
  const double bt = *beta;
  const double inv = bt > 0.0 ? 1.0 / bt : 0.0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    w[i] = w[i] * inv;
}

__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// What k_lz_init found on the diagonal that the D inner product cannot take (bits of *bad).
enum : unsigned { kDiagMissing = 1u, kDiagZero = 2u, kDiagNegative = 4u, kDiagNonFinite = 8u };

// d_i = a_ii (sum of the stored diagonal entries), dinv = 1/d; q = random; partial = sum d q^2;
// *bad |= the kinds of unusable diagonal entries met (an atomic only from a thread that met one)
__global__ __launch_bounds__(256) void k_lz_init(const int32_t* __restrict__ indptr,
                                                 const int32_t* __restrict__ indices,
                                                 const double* __restrict__ vals, int64_t n,
                                                 uint64_t seed, double* __restrict__ d,
                                                 double* __restrict__ dinv,
                                                 double* __restrict__ q,
                                                 double* __restrict__ partial,
                                                 unsigned* __restrict__ bad) {
  __shared__ double red[4];
  double acc = 0.0;
  unsigned kinds = 0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double di = 0.0;
    bool stored = false;
    for (int k = indptr[i]; k < indptr[i + 1]; ++k)
      if (indices[k] == (int32_t)i) {
        di += vals[k];
        stored = true;
      }
    if (!stored) kinds |= kDiagMissing;
    else if (di == 0.0) kinds |= kDiagZero;
    else if (di < 0.0) kinds |= kDiagNegative;
    else if (!(di <= 1.7976931348623157e308)) kinds |= kDiagNonFinite;  // NaN or inf
    d[i] = di;
    dinv[i] = 1.0 / di;
    const uint64_t r = splitmix(seed * 0x100000001B3ull + (uint64_t)i);
    const double x = (double)(r >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
    q[i] = x;
    acc += di * (x * x);
  }
  const double t = block_sum_all<256>(acc, red);
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
  if (kinds) atomicOr(bad, kinds);
}

int launch_spmv_plain(const mlamg_csr* A, const double* x, double* y, hipStream_t s);

}  // namespace mlamg

using namespace mlamg;

extern "C" int mlamg_lambda_max_dinvA(const mlamg_csr* A, int max_iter, double tol, uint64_t seed,
                                      double* lam_host, int* iters_host, void* stream) {
  MLAMG_REQUIRE(A && lam_host, "NULL argument");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "square matrix required");
  MLAMG_REQUIRE(max_iter > 0, "max_iter must be positive");
  hipStream_t s = S(stream);
  const int64_t n = A->n_rows;
  if (n == 0) {
    *lam_host = 0.0;
    if (iters_host) *iters_host = 0;
    return MLAMG_OK;
  }
  const int nbv = (int)std::min<int64_t>(1024, (n + 255) / 256);
  // No cap at n: without reorthogonalisation the Lanczos vectors lose orthogonality in finite
  // precision, and T_j may have to grow past n steps (with ghost copies of converged Ritz
  // values, which do not move its largest eigenvalue) before that eigenvalue settles.
  const int m_max = max_iter;
  const int64_t slots = (int64_t)m_max + 2;  // of alpha and of beta
  double* base = nullptr;
  MLAMG_HIP(hipMalloc(&base, sizeof(double) * (n * 6 + nbv + 2 * slots + 2)));
  struct Free {
    double* p;
    ~Free() { (void)hipFree(p); }
  } guard{base};
  double* z = base;
  double* d = z + n;
  double* dinv = d + n;
  double* Q[3] = {dinv + n, dinv + 2 * n, dinv + 3 * n};  // q_prev, q, w
  double* partial = dinv + 4 * n;
  double* alpha = partial + nbv;
  double* beta = alpha + slots;
  double* nrm0 = beta + slots;
  unsigned* bad = reinterpret_cast<unsigned*>(nrm0 + 1);
  MLAMG_HIP(hipMemsetAsync(Q[0], 0, sizeof(double) * n, s));
  MLAMG_HIP(hipMemsetAsync(beta, 0, sizeof(double) * slots, s));
  MLAMG_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(k_lz_init, dim3(nbv), dim3(256), 0, s, A->indptr, A->indices, A->data, n,
                     seed, d, dinv, Q[1], partial, bad);
  hipLaunchKernelGGL(k_reduce_to, dim3(1), dim3(1024), 0, s, partial, nbv, nrm0, 1);
  hipLaunchKernelGGL(k_lz_scale, dim3(nbv), dim3(256), 0, s, Q[1], nrm0, n);
  MLAMG_HIP(hipGetLastError());

  const int kCheck = 32;
  std::vector<double> ha(slots), hb(slots);
  double theta_prev = -1.0, theta = 0.0;
  unsigned hbad = 0;
  int j = 0;
  bool done = false;
  while (!done) {
    const int jend = std::min(m_max, j + kCheck);
    for (; j < jend; ++j) {
      MLAMG_TRY(launch_spmv_plain(A, Q[1], z, s));
      hipLaunchKernelGGL(k_lz_dot, dim3(nbv), dim3(256), 0, s, z, Q[1], n, partial);
      hipLaunchKernelGGL(k_reduce_to, dim3(1), dim3(1024), 0, s, partial, nbv, alpha + j, 0);
      // beta[j] couples q_j and q_{j-1}; beta[j+1] is the new norm
      hipLaunchKernelGGL(k_lz_update, dim3(nbv), dim3(256), 0, s, z, dinv, d, Q[1], Q[0],
                         alpha + j, beta + j, n, Q[2], partial);
      hipLaunchKernelGGL(k_reduce_to, dim3(1), dim3(1024), 0, s, partial, nbv, beta + j + 1, 1);
      hipLaunchKernelGGL(k_lz_scale, dim3(nbv), dim3(256), 0, s, Q[2], beta + j + 1, n);
      double* old = Q[0];  // q_prev <- q, q <- w, w <- (old q_prev)
      Q[0] = Q[1];
      Q[1] = Q[2];
      Q[2] = old;
    }
    MLAMG_HIP(hipGetLastError());
    MLAMG_HIP(hipMemcpyAsync(ha.data(), alpha, sizeof(double) * j, hipMemcpyDeviceToHost, s));
    MLAMG_HIP(hipMemcpyAsync(hb.data(), beta, sizeof(double) * (j + 1), hipMemcpyDeviceToHost, s));
    if (j <= kCheck)  // the first read also brings what k_lz_init saw on the diagonal
      MLAMG_HIP(hipMemcpyAsync(&hbad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    MLAMG_HIP(hipStreamSynchronize(s));
    // 1/d and the D-norm need a positive diagonal; with any other the recurrence runs on inf
    // and NaN, which the breakdown test below would take for convergence
    MLAMG_REQUIRE(!(hbad & kDiagMissing), "a row has no stored diagonal entry");
    MLAMG_REQUIRE(!(hbad & kDiagZero), "a row has a zero diagonal entry");
    MLAMG_REQUIRE(!(hbad & kDiagNegative),
                  "a row has a negative diagonal entry (positive diagonal required)");
    MLAMG_REQUIRE(!(hbad & kDiagNonFinite), "a row has a non-finite diagonal entry");
    // T_j: diagonal ha[0..j), off-diagonal hb[1..j)
    int m = j;
    bool breakdown = false;
    for (int i = 1; i <= j; ++i) {
      if (!(hb[i] > 1e-14 * std::fabs(ha[i - 1]) + 1e-300)) {
        m = i;
        breakdown = true;
        break;
      }
    }
    theta = tridiag_max_eig(ha, hb, m);
    if (breakdown || j >= m_max) done = true;
    if (theta_prev > 0.0 && std::fabs(theta - theta_prev) <= tol * std::fabs(theta)) done = true;
    theta_prev = theta;
  }
  MLAMG_REQUIRE(std::isfinite(theta), "non-finite result (non-finite matrix entries?)");
  *lam_host = theta;
  if (iters_host) *iters_host = j;
  return MLAMG_OK;
}
