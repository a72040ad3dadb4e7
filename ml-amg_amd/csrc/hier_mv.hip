// The block (n x k) V-cycle on a hierarchy handle (host side only: no kernels of its own): the
// step sequence of hier.hip's cycle_top / cycle_coarse on a row-major block of k vectors, through
// the multi-vector kernels of spmm.hip. The fusions of the single path (first sweep written by the
// restriction or the end-of-cycle residual kernel) are left out: they are the same roundings, so
// column j keeps the bits of the single-vector cycle on column j. Work buffers are k-wide copies
// of the level vectors with leading dimension k. A Gauss-Seidel level (taken once the hierarchy
// asked, mlamg_hier_set_mv_gauss_seidel) smooths its block in place with the block sweep of
// gs_mv.hip, as the single path does with gs_sweep_impl; a polynomial level (taken without a
// switch: poly.hip's block sweep is bitwise per column) with poly_sweep_mv_impl, from a zero guess
// or from the residual block it already holds exactly where the single path does. The coarsest solve is the dense inverse
// or the block PCG (pcg.hip), whose preconditioner is hier_coarse_cycle_mv on the inner
// hierarchy; the block GMRES (gmres_mv.hip) preconditions with hier_coarse_cycle_mv on the
// hierarchy itself, which then takes what mlamg_hier_vcycle_mv takes. An operator in the VECTOR format (taken once the hierarchy asked,
// mlamg_hier_set_mv_vector) goes through the canonical-order kernel of spmm_vec.hip, every other
// one through k_spmm_stream: each launch follows its own operator's format, as the single path's.
// One routine, level_mv, runs every level for both callers.
#include "hier.hpp"

#include <hip/hip_runtime.h>

using namespace mlamg;

namespace {
struct Blk {  // a row-major block of k vectors
  double* p;
  int64_t ld;
};
// an operator in the VECTOR format (mv_refusals has let it pass) is summed in the canonical
// CSR-vector order, every other one in scipy's
static inline bool canon(const mlamg_csr* A) { return A->vec_width != 0; }

struct MvLevel {
  double* x = nullptr;    // l > 0: iterate
  double* b = nullptr;    // l > 0: right-hand side
  double* r = nullptr;    // residual
  double* tmp = nullptr;  // ping-pong partner of x
};
struct MvWork {
  std::vector<MvLevel> lv;
  double* xc = nullptr;
  double* bc = nullptr;
  double* yc = nullptr;  // dense method 2: the intermediate X b
  double* r0 = nullptr;  // coarse-only hierarchy: residual of the history
  int k = 0;
  hipStream_t s = nullptr;
  // stop flag of every launch: hier_coarse_cycle_mv's caller's; none for mlamg_hier_vcycle_mv
  const int32_t* done = nullptr;
  // level l as a coarse level (l = lv.size(): the coarsest solve): its iterate and right-hand side
  Blk iterate(size_t l) const { return {l < lv.size() ? lv[l].x : xc, k}; }
  double* rhs(size_t l) const { return l < lv.size() ? lv[l].b : bc; }
  // The SpMM-family launches of the cycle (r, bn: leading dimension k). The summation order is
  // decided here: every launch follows its own operator's format.
  int residual(const mlamg_csr* A, const double* B, int64_t ldb, Blk x, double* r) const {
    return residual_mv(A, B, ldb, x.p, x.ld, r, k, k, s, done, canon(A));
  }
  int jacobi(const Level& L, const double* B, int64_t ldb, Blk in, Blk out) const {
    return jacobi_sweep_mv(L.A, L.dinv, B, ldb, in.p, in.ld, out.p, out.ld, k, s, done,
                           canon(L.A));
  }
  int restrict_to(const mlamg_csr* R, const double* r, double* bn) const {
    return spmm_set_mv(R, r, k, bn, k, k, 1.0, 0.0, s, done, canon(R));
  }
  int prolong_add(const mlamg_csr* P, Blk e, Blk x) const {
    return spmm_add_mv(P, e.p, e.ld, x.p, x.ld, k, s, done, canon(P));
  }
};

static int mv_unsupported(const char* why, const char* who = "mlamg_hier_vcycle_mv") {
  set_error(std::string(who) + ": " + why);
  return MLAMG_EUNSUPPORTED;
}

// what the block cycle cannot run (MLAMG_EUNSUPPORTED, the message names it); pcg_ok: a PCG
// coarsest solve is taken (the block PCG), else the coarsest solve must be the dense inverse;
// gs_ok: Gauss-Seidel levels are taken (the block sweep, gs_mv.hip); vec_ok: VECTOR-format
// operators are taken (the canonical-order kernel, spmm_vec.hip)
static int mv_refusals(const mlamg_hier* H, bool pcg_ok, bool gs_ok, bool vec_ok,
                       const char* who) {
  if (H->pcg && !pcg_ok)
    return mv_unsupported("the coarse solve is PCG (dense coarse solves only)", who);
  if (H->gm_inner)
    return mv_unsupported("the coarse solve is GMRES (dense coarse solves only)", who);
  for (const Level& L : H->lv) {
    if (L.gs && !gs_ok)
      return mv_unsupported("a level uses a Gauss-Seidel smoother (weighted Jacobi only)", who);
    if (L.fac_A) return mv_unsupported("a level uses a factored prolongation", who);
    if (!vec_ok && (L.A->vec_width || L.P->vec_width || L.R->vec_width))
      return mv_unsupported("an operator is in the VECTOR format, whose row order is not scipy's",
                            who);
  }
  return MLAMG_OK;
}

// the layout of H->mv_mem: k-wide level blocks (level 0 iterates in the caller's X and reads the
// caller's B; as a coarse level, hier_coarse_cycle_mv, it has an iterate of its own: level0_x),
// then the coarse blocks; returns the bytes needed
static size_t mv_layout(const mlamg_hier* H, int k, MvWork* W, char* base, bool level0_x) {
  Carver c{base};
  auto take = [&](int64_t n) { return c.take(std::max<int64_t>(n, 1) * k); };
  const size_t nl = H->lv.size();
  const int64_t nc = coarse_rows(H);
  W->lv.resize(nl);
  for (size_t l = 0; l < nl; ++l) {
    if (l > 0 || level0_x) W->lv[l].x = take(H->lv[l].n);
    if (l > 0) W->lv[l].b = take(H->lv[l].n);
    W->lv[l].r = take(H->lv[l].n);
    W->lv[l].tmp = take(H->lv[l].n);
  }
  W->xc = take(nc);
  W->bc = take(nc);
  W->yc = take(nc);
  if (nl == 0) W->r0 = take(nc);
  return c.off;
}

static int mv_workspace(mlamg_hier* H, int k, hipStream_t s, const int32_t* done, MvWork* W,
                        bool level0_x) {
  W->k = k;
  W->s = s;
  W->done = done;
  const size_t total = mv_layout(H, k, W, nullptr, level0_x);
  if (H->mv_bytes < total) {
    if (H->mv_mem) (void)hipFree(H->mv_mem);  // ordered after every earlier use (cache semantics)
    H->mv_mem = nullptr;
    H->mv_bytes = 0;
    MLAMG_HIP(hipMalloc(&H->mv_mem, total));
    H->mv_bytes = total;
  }
  mv_layout(H, k, W, static_cast<char*>(H->mv_mem), level0_x);
  return MLAMG_OK;
}

// nu smoothing sweeps on the iterate in `cur`. A Jacobi sweep writes the partner `other` and the
// two change roles, so `other` stays the one of the pair that `cur` is not; Gauss-Seidel sweeps
// in place.
static int smooth(const MvWork& W, const Level& L, const double* B, int64_t ldb, Blk& cur,
                  Blk& other, int nu, bool zero = false, const double* r_ready = nullptr) {
  if (L.gs) return gs_sweep_mv_impl(L.gs, cur.p, cur.ld, B, ldb, W.k, nu, W.done, W.s);
  if (L.poly)  // in place; zero: cur is not read; r_ready (ld = k): B - A cur, not recomputed
    return poly_sweep_mv_impl(L.poly, cur.p, cur.ld, B, ldb, W.k, nu * L.poly_iters, zero,
                              r_ready, W.k, W.done, W.s, canon(L.A));
  for (int i = 0; i < nu; ++i) {
    MLAMG_TRY(W.jacobi(L, B, ldb, cur, other));
    std::swap(cur, other);
  }
  return MLAMG_OK;
}

// how a level starts: from a zero guess (every coarse level; x and B are then work blocks with
// ld = k), or from the iterate in x, without or with B - A x already in the level's residual block
enum Start { ZERO_GUESS, ITERATE, ITERATE_R };

// One V-cycle of level l on (B, ldb) with the iterate in x; the ping-pong partner is the level's
// tmp block. l = lv.size() is the coarsest solve (dense inverse or block PCG), straight into x.
// The block that holds the result (x or the partner) is returned through `res`.
static int level_mv(mlamg_hier* H, MvWork& W, size_t l, const double* B, int64_t ldb, Blk x,
                    Start start, Blk* res) {
  const int k = W.k;
  hipStream_t s = W.s;
  *res = x;
  if (l == H->lv.size()) {
    if (H->D) return dense_solve_mv(H->D, B, ldb, x.p, x.ld, k, W.yc, s, W.done);
    return pcg_solve_mv_impl(H->pcg, B, ldb, x.p, x.ld, k, s);
  }
  const Level& L = H->lv[l];
  const MvLevel& M = W.lv[l];
  Blk cur = x, other{M.tmp, k};
  const int nu = H->nu_pre;
  // the first Jacobi sweep is elementwise: x = Dinv_w B from a zero guess, x += Dinv_w r from an
  // iterate (same roundings as a sweep). Gauss-Seidel has no such shortcut and reads no residual
  const bool gs_pre = L.gs && nu > 0, jacobi_pre = !L.gs && !L.poly && nu > 0;
  if (L.poly && nu > 0) {
    // the single path's steps (cycle_coarse / cycle_top): a zero guess is not read, a residual the
    // cycle holds (ITERATE_R) starts the first iteration
    MLAMG_TRY(smooth(W, L, B, ldb, cur, other, nu, start == ZERO_GUESS,
                     start == ITERATE_R ? M.r : nullptr));
    MLAMG_TRY(W.residual(L.A, B, ldb, cur, M.r));
  } else if (start == ZERO_GUESS) {
    if (jacobi_pre) {
      MLAMG_TRY(diag_mv(cur.p, cur.ld, L.dinv, B, ldb, L.n, k, 1, s, W.done));
    } else {
      const size_t bytes = sizeof(double) * (size_t)L.n * (size_t)k;
      MLAMG_HIP(hipMemsetAsync(cur.p, 0, bytes, s));
      if (!gs_pre) MLAMG_HIP(hipMemcpyAsync(M.r, B, bytes, hipMemcpyDeviceToDevice, s));  // r = B
    }
  } else {
    if (start != ITERATE_R && !gs_pre) MLAMG_TRY(W.residual(L.A, B, ldb, cur, M.r));
    if (jacobi_pre) MLAMG_TRY(diag_mv(cur.p, cur.ld, L.dinv, M.r, k, L.n, k, 0, s, W.done));
  }
  if (nu > 0 && !L.poly) {
    MLAMG_TRY(smooth(W, L, B, ldb, cur, other, gs_pre ? nu : nu - 1));
    MLAMG_TRY(W.residual(L.A, B, ldb, cur, M.r));
  }
  double* bn = W.rhs(l + 1);
  MLAMG_TRY(W.restrict_to(L.R, M.r, bn));
  Blk e;
  MLAMG_TRY(level_mv(H, W, l + 1, bn, k, W.iterate(l + 1), ZERO_GUESS, &e));
  MLAMG_TRY(W.prolong_add(L.P, e, cur));
  MLAMG_TRY(smooth(W, L, B, ldb, cur, other, H->nu_post));
  *res = cur;
  return MLAMG_OK;
}
}  // namespace

namespace mlamg {
int hier_coarse_cycle_mv(mlamg_hier* H, const double* B, double** X_out, int k, hipStream_t s,
                         const int32_t* done, bool outer) {
  if (outer) {
    MLAMG_TRY(mv_refusals(H, true, H->mv_gs, H->mv_vec, "block cycle of mlamg_gmres_mv"));
  } else {
    MLAMG_TRY(
        mv_refusals(H, false, false, false, "block cycle of a Krylov solver's inner hierarchy"));
  }
  MLAMG_TRY(hier_prepare(H));
  MvWork W;
  MLAMG_TRY(mv_workspace(H, k, s, done, &W, true));
  Blk res;
  MLAMG_TRY(level_mv(H, W, 0, B, k, W.iterate(0), ZERO_GUESS, &res));
  *X_out = res.p;
  return MLAMG_OK;
}
}  // namespace mlamg

extern "C" {

int mlamg_hier_vcycle_mv(mlamg_hier* H, const double* B, int64_t ldb, double* X, int64_t ldx,
                         int k, int n_cycles, int norm_mode, int remove_mean, double* hist,
                         void* stream) {
  MLAMG_REQUIRE(H && X, "NULL argument");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k && (!B || ldb >= k), "leading dimension < k");
  MLAMG_REQUIRE(B != X, "B and X must differ");
  MLAMG_REQUIRE(n_cycles >= 0, "n_cycles < 0");
  MLAMG_REQUIRE(norm_mode == 0 || norm_mode == 1, "norm_mode must be 0 (residual) or 1 (x)");
  MLAMG_TRY(mv_refusals(H, true, H->mv_gs, H->mv_vec, "mlamg_hier_vcycle_mv"));
  MLAMG_TRY(hier_prepare(H));
  hipStream_t s = S(stream);
  MvWork W;
  MLAMG_TRY(mv_workspace(H, k, s, nullptr, &W, false));
  // the operator, size and residual block of the history: the finest level's, or, for a
  // coarse-only hierarchy (X = A^-1 B each cycle), the coarsest operator's, which is summed in
  // scipy's order whatever its format, as the block PCG sums it
  const bool levels = !H->lv.empty();
  const mlamg_csr* A = levels ? H->lv[0].A : H->Ac;
  const int64_t n = levels ? H->lv[0].n : coarse_rows(H);
  double* r = levels ? W.lv[0].r : W.r0;
  if (!levels) {
    if (!B) {
      MLAMG_HIP(hipMemsetAsync(W.bc, 0, sizeof(double) * (size_t)std::max<int64_t>(n, 1) * k, s));
      B = W.bc;
      ldb = k;
    }
    if (hist && norm_mode == 0 && !A)
      return mv_unsupported("a coarse-only hierarchy without its operator has no residual norm");
  }
  bool have_r = false;  // r == B - A X (the end-of-cycle residual, reused by the next sweep)
  for (int c = 0; c < n_cycles; ++c) {
    Blk res;
    MLAMG_TRY(level_mv(H, W, 0, B, ldb, Blk{X, ldx}, have_r ? ITERATE_R : ITERATE, &res));
    if (res.p != X && n > 0)
      MLAMG_HIP(hipMemcpy2DAsync(X, sizeof(double) * ldx, res.p, sizeof(double) * res.ld,
                                 sizeof(double) * k, n, hipMemcpyDeviceToDevice, s));
    if (remove_mean) MLAMG_TRY(remove_mean_mv(X, ldx, n, k, s));
    have_r = false;
    if (hist && norm_mode == 0) {
      MLAMG_TRY(residual_mv(A, B, ldb, X, ldx, r, k, k, s, W.done, levels && canon(A)));
      MLAMG_TRY(norm2_mv(r, k, n, k, hist + (int64_t)c * k, s));
      have_r = true;
    } else if (hist) {
      MLAMG_TRY(norm2_mv(X, ldx, n, k, hist + (int64_t)c * k, s));
    }
  }
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_hier_set_mv_gauss_seidel(mlamg_hier* H, int on) {
  MLAMG_REQUIRE(H, "H is NULL");
  H->mv_gs = on != 0;
  return MLAMG_OK;
}

int mlamg_hier_set_mv_vector(mlamg_hier* H, int on) {
  MLAMG_REQUIRE(H, "H is NULL");
  H->mv_vec = on != 0;
  return MLAMG_OK;
}

}  // extern "C"
