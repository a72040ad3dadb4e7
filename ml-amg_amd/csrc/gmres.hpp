// What the single-vector GMRES (gmres.hip) and the block one (gmres_mv.hip) share: the launch
// shape of the Gram-Schmidt reductions, and the one-thread Hessenberg work of an Arnoldi step.
// Column j of the block solve has the bits of the single solve because both run the code below.
#pragma once
#include "common.hpp"
#include "reduce.hpp"

#include <cmath>

namespace mlamg {

constexpr int kGmThreads = 256;
constexpr int kGmMaxBlocks = 1024;

// sum of np partials by a whole workgroup of kGmThreads, every thread gets it; behind a barrier,
// because red may still be read from the sum before
__device__ __forceinline__ double gm_total(const double* __restrict__ partial, int np,
                                           double* red) {
  __syncthreads();
  return partials_total_all<kGmThreads>(partial, np, red);
}

// LAPACK dlartg (3.10+, the safe-scaling version scipy's get_lapack_funcs('lartg') binds):
// c f + s g = r, -s f + c g = 0
__host__ __device__ inline void lartg(double f, double g, double* c, double* s, double* r) {
  if (g == 0.0) {
    *c = 1.0;
    *s = 0.0;
    *r = f;
  } else if (f == 0.0) {
    *c = 0.0;
    *s = g > 0 ? 1.0 : -1.0;
    *r = fabs(g);
  } else {
    const double d = sqrt(f * f + g * g);
    *c = fabs(f) / d;
    *r = f > 0 ? d : -d;
    *s = g / *r;
  }
}

// One Arnoldi step's small-matrix work, by one thread — what scipy's numpy code does with the
// column, the same operations in the same order (so the same bits): Hessenberg column from the
// MGS coefficients scal[0..col] and the norms sqrt(w0), sqrt(w1) of w before and after the
// projections, exact-solution test, the past rotations, a new rotation (lartg), the rotated
// right-hand side and the preconditioned residual estimate. Returns the inner stop
// (presid <= ptol or breakdown).
// st: [0] presid, [1] h1 (the scale of v_{col+1}), [2] breakdown, [3] last column, [4] steps,
// [5] ||w||^2 before the projections (h0^2).
__device__ __forceinline__ bool gm_arnoldi_step(int col, int ldh, const double* __restrict__ scal,
                                                double w0, double w1, double* __restrict__ Hd,
                                                double* __restrict__ giv, double* __restrict__ S,
                                                double* __restrict__ st, double eps, double ptol,
                                                double bnrm2, double* __restrict__ hist,
                                                int hist_cap) {
  st[5] = w0;
  auto H = [&](int c, int k) -> double& { return Hd[(size_t)c * ldh + k]; };
  const double h0 = sqrt(w0);
  for (int k = 0; k <= col; ++k) H(col, k) = scal[k];
  const double h1 = sqrt(w1);
  H(col, col + 1) = h1;
  bool breakdown = false;
  if (h1 <= eps * h0) {  // exact solution indicator
    H(col, col + 1) = 0.0;
    breakdown = true;
  }
  st[1] = h1;
  for (int k = 0; k < col; ++k) {  // past rotations
    const double c = giv[2 * k], sn = giv[2 * k + 1];
    const double n0 = H(col, k), n1 = H(col, k + 1);
    H(col, k) = c * n0 + sn * n1;
    H(col, k + 1) = -sn * n0 + c * n1;
  }
  double c, sn, mag;
  lartg(H(col, col), H(col, col + 1), &c, &sn, &mag);
  giv[2 * col] = c;
  giv[2 * col + 1] = sn;
  H(col, col) = mag;
  H(col, col + 1) = 0.0;
  const double t2 = -sn * S[col];
  S[col] = c * S[col];
  S[col + 1] = t2;
  const double presid = fabs(t2);
  const int steps = (int)st[4];
  if (hist && steps < hist_cap) hist[steps] = presid / bnrm2;
  st[0] = presid;
  st[2] = breakdown ? 1.0 : 0.0;
  st[3] = (double)col;
  st[4] = (double)(steps + 1);
  return presid <= ptol || breakdown;
}

// The restart boundary's small triangular solve (host): y = R^-1 S on the leading col + 1 rotated
// Hessenberg columns h (column c at h + c ldh), scipy's back substitution
inline void gm_small_solve(const double* h, int ldh, double* S, int col, double* y) {
  auto H = [&](int c, int k) -> double { return h[(size_t)c * ldh + k]; };
  if (H(col, col) == 0.0) S[col] = 0.0;
  for (int k = 0; k <= col; ++k) y[k] = S[k];
  for (int k = col; k > 0; --k) {
    if (y[k] != 0.0) {
      y[k] /= H(k, k);
      const double t = y[k];
      for (int j = 0; j < k; ++j) y[j] -= t * H(k, j);
    }
  }
  if (y[0] != 0.0) y[0] /= H(0, 0);
}

}  // namespace mlamg
