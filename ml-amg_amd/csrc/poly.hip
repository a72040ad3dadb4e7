// Polynomial (Chebyshev) smoother: pyamg relaxation.polynomial on the device.
//
// One iteration with the coefficients c[0..m) (c[0] on the highest power, pyamg's order) is
//     r = b - A x;  h = c[0] r;  for i in 1..m-1: h = c[i] r + A h;  x = x + h
// with every operation rounded on its own: A h is the storage format's row sum (mlamg_spmv's),
// c[i] r one multiply, the sum one add, x + h one add. Each line is one SpMV-family launch whose
// epilogue (spmv.hip EPI_POLY, spmm_epi.hpp MV_POLY) does the vector work, so an iteration is m
// launches and m passes over A and nothing else: the first launch writes r and h = c[0] r
// together, the last one adds into x in place (x is not its SpMV operand). From a known-zero x the
// first pass goes: r = b (b - A 0 bit for bit, for finite A), h = c[0] b is one elementwise
// launch, and the last launch forms +0.0 + h (the bits of the general path on an all-zero x).
// Where the caller already holds r = b - A x (the V-cycle executors do), the first pass is that
// elementwise launch on r as well. A one-coefficient sweep cannot write x while the launch gathers
// from it: it goes through h and a copy.
//
// This unit is host code plus the one elementwise kernel; the handle owns r and the two h buffers
// (and their k-wide copies for the block sweep, grown on demand outside stream captures).
#include "common.hpp"

#include <cmath>

struct mlamg_poly {
  const mlamg_csr* A = nullptr;
  int64_t n = 0;
  std::vector<double> c;  // host: launch scalars
  double* r = nullptr;
  double* h0 = nullptr;
  double* h1 = nullptr;
  // block work space: r, h0, h1 as n x mv_k blocks (leading dimension = the sweep's k)
  mutable double* mv = nullptr;
  mutable int mv_k = 0;
};

namespace mlamg {

enum PolyEw : int { PW_SCALE = 0, PW_ADD = 1, PW_ZERO = 2, PW_COPY = 3 };

// out[i, c] = alpha R[i, c] (SCALE), Xin[i, c] + alpha R[i, c] (ADD), +0.0 + alpha R[i, c] (ZERO:
// the sweep's x + h on an all-zero x) or R[i, c] (COPY); R NULL: +0.0. One element per thread.
__global__ __launch_bounds__(256) void k_poly_ew(double* out, int64_t ldo,
                                                 const double* R, int64_t ldr, double alpha,
                                                 const double* Xin, int64_t ldxin, int mode,
                                                 int64_t n, int k,
                                                 const int32_t* __restrict__ done) {
  const int64_t w = blockIdx.x * 256ll + threadIdx.x;
  if (w >= n * k || (done && *done)) return;
  const int64_t i = w / k;
  const int c = (int)(w - i * k);
  const double r = R ? R[i * ldr + c] : 0.0;
  double o;
  if (mode == PW_COPY) {
    o = r;
  } else {
    const double h = alpha * r;
    o = mode == PW_ADD ? Xin[i * ldxin + c] + h : (mode == PW_ZERO ? 0.0 + h : h);
  }
  out[i * ldo + c] = o;
}

static int poly_ew(double* out, int64_t ldo, const double* R, int64_t ldr, double alpha,
                   const double* Xin, int64_t ldxin, int mode, int64_t n, int k,
                   const int32_t* done, hipStream_t s) {
  if (n == 0) return MLAMG_OK;
  const int64_t nb = (n * k + 255) / 256;
  hipLaunchKernelGGL(k_poly_ew, dim3((unsigned)nb), dim3(256), 0, s, out, ldo, R, ldr, alpha, Xin,
                     ldxin, mode, n, k, done);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int64_t poly_rows(const mlamg_poly* S) { return S->n; }
int poly_terms(const mlamg_poly* S) { return (int)S->c.size(); }

int poly_sweep_impl(const mlamg_poly* S, double* x, const double* b, int iterations, bool x_is_zero,
                    const double* r_ready, const int32_t* done, hipStream_t s) {
  const mlamg_csr* A = S->A;
  const int m = (int)S->c.size();
  const double* c = S->c.data();
  const int64_t n = S->n;
  for (int it = 0; it < iterations; ++it) {
    const bool zero = x_is_zero && it == 0;
    const double* have = (!zero && it == 0) ? r_ready : nullptr;
    if (m == 1) {
      if (zero) {
        MLAMG_TRY(poly_ew(x, 1, b, 1, c[0], nullptr, 1, PW_ZERO, n, 1, done, s));
      } else if (have) {
        MLAMG_TRY(poly_ew(x, 1, have, 1, c[0], x, 1, PW_ADD, n, 1, done, s));
      } else {
        MLAMG_TRY(poly_first(A, b, x, nullptr, c[0], x, S->h0, done, s));
        MLAMG_TRY(poly_ew(x, 1, S->h0, 1, 0.0, nullptr, 1, PW_COPY, n, 1, done, s));
      }
      continue;
    }
    const double* r = S->r;
    if (zero || have) {
      r = zero ? b : have;
      MLAMG_TRY(poly_ew(S->h0, 1, r, 1, c[0], nullptr, 1, PW_SCALE, n, 1, done, s));
    } else {
      MLAMG_TRY(poly_first(A, b, x, S->r, c[0], nullptr, S->h0, done, s));
    }
    double* hin = S->h0;
    double* hout = S->h1;
    for (int i = 1; i + 1 < m; ++i) {
      MLAMG_TRY(poly_step(A, c[i], r, hin, false, nullptr, hout, done, s));
      std::swap(hin, hout);
    }
    MLAMG_TRY(poly_step(A, c[m - 1], r, hin, true, zero ? nullptr : x, x, done, s));
  }
  return MLAMG_OK;
}

int poly_reserve_mv(const mlamg_poly* S, int k) {
  if (S->mv_k >= k) return MLAMG_OK;
  if (S->mv) (void)hipFree(S->mv);  // ordered after every earlier use (cache semantics)
  S->mv = nullptr;
  S->mv_k = 0;
  const size_t blk = (size_t)std::max<int64_t>(S->n, 1) * (size_t)k;
  MLAMG_HIP(hipMalloc(&S->mv, sizeof(double) * 3 * blk));
  S->mv_k = k;
  return MLAMG_OK;
}

int poly_sweep_mv_impl(const mlamg_poly* S, double* X, int64_t ldx, const double* B, int64_t ldb,
                       int k, int iterations, bool x_is_zero, const double* R_ready, int64_t ldr,
                       const int32_t* done, hipStream_t s, bool canon) {
  const mlamg_csr* A = S->A;
  const int m = (int)S->c.size();
  const double* c = S->c.data();
  const int64_t n = S->n;
  if (iterations <= 0) return MLAMG_OK;
  if (S->mv_k < k) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    MLAMG_HIP(hipStreamIsCapturing(s, &st));
    MLAMG_REQUIRE(st == hipStreamCaptureStatusNone,
                  "the block work space cannot grow inside a stream capture (sweep once before)");
    MLAMG_TRY(poly_reserve_mv(S, k));
  }
  // blocks of the sweep's own width, so that k = 2, 4, ... keep the 16-byte accesses
  const size_t blk = (size_t)std::max<int64_t>(n, 1) * (size_t)k;
  double* Rw = S->mv;
  double* H0 = S->mv + blk;
  double* H1 = S->mv + 2 * blk;
  for (int it = 0; it < iterations; ++it) {
    const bool zero = x_is_zero && it == 0;
    const double* have = (!zero && it == 0) ? R_ready : nullptr;
    if (m == 1) {
      if (zero) {
        MLAMG_TRY(poly_ew(X, ldx, B, ldb, c[0], nullptr, 0, PW_ZERO, n, k, done, s));
      } else if (have) {
        MLAMG_TRY(poly_ew(X, ldx, have, ldr, c[0], X, ldx, PW_ADD, n, k, done, s));
      } else {
        MLAMG_TRY(poly_first_mv(A, B, ldb, X, ldx, nullptr, 0, c[0], X, ldx, H0, k, k, s, done,
                                canon));
        MLAMG_TRY(poly_ew(X, ldx, H0, k, 0.0, nullptr, 0, PW_COPY, n, k, done, s));
      }
      continue;
    }
    const double* R = Rw;
    int64_t lr = k;
    if (zero || have) {
      R = zero ? B : have;
      lr = zero ? ldb : ldr;
      MLAMG_TRY(poly_ew(H0, k, R, lr, c[0], nullptr, 0, PW_SCALE, n, k, done, s));
    } else {
      MLAMG_TRY(poly_first_mv(A, B, ldb, X, ldx, Rw, k, c[0], nullptr, 0, H0, k, k, s, done,
                              canon));
    }
    double* hin = H0;
    double* hout = H1;
    for (int i = 1; i + 1 < m; ++i) {
      MLAMG_TRY(poly_step_mv(A, c[i], R, lr, hin, k, false, nullptr, 0, hout, k, k, s, done,
                             canon));
      std::swap(hin, hout);
    }
    MLAMG_TRY(poly_step_mv(A, c[m - 1], R, lr, hin, k, true, zero ? nullptr : X, ldx, X, ldx, k, s,
                           done, canon));
  }
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_poly_create(const mlamg_csr* A, const double* coeffs_host, int n_coeffs,
                      mlamg_poly** out, void* stream) {
  MLAMG_REQUIRE(A && coeffs_host && out, "NULL argument");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "the operator must be square");
  MLAMG_REQUIRE(n_coeffs >= 1, "n_coeffs < 1");
  for (int i = 0; i < n_coeffs; ++i)
    MLAMG_REQUIRE(std::isfinite(coeffs_host[i]), "a coefficient is not finite");
  mlamg_poly* S = new mlamg_poly();
  S->A = A;
  S->n = A->n_rows;
  S->c.assign(coeffs_host, coeffs_host + n_coeffs);
  const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(S->n, 1);
  double** bufs[3] = {&S->r, &S->h0, &S->h1};
  for (double** p : bufs) {
    if (hipMalloc(p, bytes) != hipSuccess) {
      (void)mlamg_poly_destroy(S);
      set_error("mlamg_poly_create: device allocation failed");
      return MLAMG_ENOMEM;
    }
  }
  (void)stream;
  *out = S;
  return MLAMG_OK;
}

int mlamg_poly_destroy(mlamg_poly* S) {
  if (!S) return MLAMG_OK;
  if (S->r) (void)hipFree(S->r);
  if (S->h0) (void)hipFree(S->h0);
  if (S->h1) (void)hipFree(S->h1);
  if (S->mv) (void)hipFree(S->mv);
  delete S;
  return MLAMG_OK;
}

int mlamg_poly_info(const mlamg_poly* S, int64_t* rows, int* n_coeffs) {
  MLAMG_REQUIRE(S, "S is NULL");
  if (rows) *rows = S->n;
  if (n_coeffs) *n_coeffs = (int)S->c.size();
  return MLAMG_OK;
}

int mlamg_poly_sweep(const mlamg_poly* S, double* x, const double* b, int iterations,
                     int x_is_zero, void* stream) {
  MLAMG_REQUIRE(S && (S->n == 0 || x), "NULL argument");
  MLAMG_REQUIRE(iterations >= 0, "iterations < 0");
  MLAMG_REQUIRE(b != x, "b and x must differ");
  return poly_sweep_impl(S, x, b, iterations, x_is_zero != 0, nullptr, nullptr, ::mlamg::S(stream));
}

int mlamg_poly_sweep_mv(const mlamg_poly* S, double* X, int64_t ldx, const double* B, int64_t ldb,
                        int k, int iterations, int x_is_zero, void* stream) {
  MLAMG_REQUIRE(S && (S->n == 0 || X), "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k && (!B || ldb >= k), "leading dimension < k");
  MLAMG_REQUIRE(iterations >= 0, "iterations < 0");
  MLAMG_REQUIRE(B != X, "B and X must differ");
  return poly_sweep_mv_impl(S, X, ldx, B, ldb, k, iterations, x_is_zero != 0, nullptr, 0, nullptr,
                            ::mlamg::S(stream), S->A->vec_width != 0);
}

}  // extern "C"
