// The epilogues of the multi-vector SpMM kernels, shared by the scipy-order kernel (spmm.hip
// k_spmm_stream) and the canonical-order one (spmm_vec.hip k_spmm_vcan): the single-vector
// epilogues (spmv.hip epi_store) on a pair of adjacent columns.
#pragma once
#include "common.hpp"

#include <hip/hip_runtime.h>

namespace mlamg {

enum MvOp : int { MV_AXPBY = 0, MV_RESID = 1, MV_JACOBI = 2, MV_ADD = 3, MV_POLY = 4 };

struct EpiMV {
  int op;
  double alpha, beta;   // AXPBY
  const double* B;      // RESID / JACOBI right-hand side (NULL: +0.0)
  int64_t ldb;
  const double* Xin;    // JACOBI: old iterate (the SpMM operand itself)
  int64_t ldxin;
  const double* dinv;   // JACOBI: one weight per row, shared by the columns
  double* Y;            // output (AXPBY with beta != 0 and ADD also read it)
  int64_t ldy;
  const int32_t* done;  // nullable stop flag: raised, the launch does nothing
  // POLY (spmv.hip EPI_POLY per column): Y = alpha B + A X, with Xin set (or beta != 0 for an
  // all-zero Xin that is not read) Y = Xin + (alpha B + A X); with H set the sweep's first launch
  // Y = R = B - A X (Y nullable), H = alpha R, with Xin set H = Xin + alpha R (H is not X)
  double* H;
  int64_t ldh;
};

// two adjacent columns at p (the second only when `two`)
template <bool VEC>
__device__ __forceinline__ void ld2(const double* __restrict__ p, bool two, double& a, double& b) {
  if constexpr (VEC) {
    if (two) {
      const double2 t = *reinterpret_cast<const double2*>(p);
      a = t.x;
      b = t.y;
    } else {
      a = p[0];
      b = 0.0;
    }
  } else {
    a = p[0];
    b = two ? p[1] : 0.0;
  }
}

template <bool VEC>
__device__ __forceinline__ void st2(double* __restrict__ p, bool two, double a, double b) {
  if constexpr (VEC) {
    if (two) {
      *reinterpret_cast<double2*>(p) = make_double2(a, b);
    } else {
      p[0] = a;
    }
  } else {
    p[0] = a;
    if (two) p[1] = b;
  }
}

// the single-vector epilogues (spmv.hip epi_store) on the column pair (c, c + 1) of `row`
template <bool VEC>
__device__ __forceinline__ void epi_mv(int64_t row, int c, bool two, double s0, double s1,
                                       const EpiMV& e) {
  double* y = e.Y + row * e.ldy + c;
  double o0, o1;
  if (e.op == MV_AXPBY) {
    if (e.beta == 0.0) {
      o0 = (e.alpha == 1.0) ? s0 : e.alpha * s0;
      o1 = (e.alpha == 1.0) ? s1 : e.alpha * s1;
    } else {
      double y0, y1;
      ld2<VEC>(y, two, y0, y1);
      o0 = e.alpha * s0 + e.beta * y0;
      o1 = e.alpha * s1 + e.beta * y1;
    }
  } else if (e.op == MV_RESID) {
    double b0 = 0.0, b1 = 0.0;  // B NULL: a zero right-hand side (+0.0: the same bits)
    if (e.B) ld2<VEC>(e.B + row * e.ldb + c, two, b0, b1);
    o0 = b0 - s0;
    o1 = b1 - s1;
  } else if (e.op == MV_JACOBI) {
    double b0 = 0.0, b1 = 0.0, x0, x1;
    if (e.B) ld2<VEC>(e.B + row * e.ldb + c, two, b0, b1);
    ld2<VEC>(e.Xin + row * e.ldxin + c, two, x0, x1);
    const double d = e.dinv[row];
    const double r0 = b0 - s0, r1 = b1 - s1;
    o0 = x0 + d * r0;
    o1 = x1 + d * r1;
  } else if (e.op == MV_POLY) {
    double b0 = 0.0, b1 = 0.0, x0 = 0.0, x1 = 0.0;
    if (e.B) ld2<VEC>(e.B + row * e.ldb + c, two, b0, b1);
    if (e.Xin) ld2<VEC>(e.Xin + row * e.ldxin + c, two, x0, x1);
    if (e.H) {
      const double r0 = b0 - s0, r1 = b1 - s1;
      if (e.Y) st2<VEC>(y, two, r0, r1);
      const double h0 = e.alpha * r0, h1 = e.alpha * r1;
      st2<VEC>(e.H + row * e.ldh + c, two, e.Xin ? x0 + h0 : h0, e.Xin ? x1 + h1 : h1);
      return;
    }
    const double t0 = e.alpha * b0, t1 = e.alpha * b1;
    const double h0 = t0 + s0, h1 = t1 + s1;
    const bool acc = e.Xin || e.beta != 0.0;
    o0 = acc ? x0 + h0 : h0;
    o1 = acc ? x1 + h1 : h1;
  } else {  // MV_ADD
    double y0, y1;
    ld2<VEC>(y, two, y0, y1);
    o0 = y0 + s0;
    o1 = y1 + s1;
  }
  st2<VEC>(y, two, o0, o1);
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// whether every block an SpMM launch touches allows 16-byte accesses
static inline bool mv_vec16(const double* X, int64_t ldx, const EpiMV& ep) {
  bool vec = al16(X) && !(ldx & 1) && al16(ep.Y) && !(ep.ldy & 1);
  if (ep.B) vec = vec && al16(ep.B) && !(ep.ldb & 1);
  if (ep.op == MV_JACOBI || (ep.op == MV_POLY && ep.Xin))
    vec = vec && al16(ep.Xin) && !(ep.ldxin & 1);
  if (ep.op == MV_POLY && ep.H) vec = vec && al16(ep.H) && !(ep.ldh & 1);
  return vec;
}

// one canonical-order SpMM launch with epilogue `ep` (spmm_vec.hip; arguments already validated)
int launch_spmm_vcan(const mlamg_csr* A, const double* X, int64_t ldx, int k, const EpiMV& ep,
                     hipStream_t s);


// what the C entries mlamg_residual_mv / mlamg_jacobi_mv and their _vec twins run after their own
// argument checks (spmm.hip)
int residual_mv_run(const mlamg_csr* A, const double* B, int64_t ldb, const double* X, int64_t ldx,
                    double* R, int64_t ldr, int k, double* norms, hipStream_t s, bool canon);
int jacobi_mv_run(const mlamg_csr* A, const double* dinv_w, const double* B, int64_t ldb, double* X,
                  int64_t ldx, double* X_tmp, int64_t ldt, int k, int nu, hipStream_t s,
                  bool canon);

}  // namespace mlamg
