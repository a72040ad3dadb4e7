// What the single-vector executor (hier.hip) and the block (n x k) one (hier_mv.hip) share: the
// hierarchy handle, its levels, and the helpers both call.
#pragma once
#include "cycle.hpp"

namespace mlamg {
struct Level {
  const mlamg_csr* A = nullptr;
  const double* dinv = nullptr;
  const mlamg_csr* P = nullptr;
  const mlamg_csr* R = nullptr;
  int64_t n = 0;
  double* x = nullptr;    // l > 0: iterate
  double* b = nullptr;    // l > 0: right-hand side
  double* r = nullptr;    // residual
  double* tmp = nullptr;  // ping-pong partner of x
  const mlamg_gs* gs = nullptr;  // Gauss-Seidel smoother (in place) instead of weighted Jacobi
  // polynomial smoother (in place; poly.hip) instead: poly_iters iterations per sweep. A level has
  // at most one of gs / poly
  const mlamg_poly* poly = nullptr;
  int poly_iters = 1;
  // factored prolongation (opt-in, mlamg_hier_set_factored_prolong): x += t - (w D^-1) A t with
  // t = Agg e, through fac_A (this level's A in the uniform row-pair format), instead of x += P e
  const mlamg_csr* fac_A = nullptr;
  const int32_t* fac_agg = nullptr;
  const double* fac_dinv = nullptr;
};
}  // namespace mlamg

struct mlamg_hier {
  std::vector<mlamg::Level> lv;
  const mlamg_csr* Ac = nullptr;
  const mlamg_dense* D = nullptr;
  mlamg_pcg* pcg = nullptr;  // coarse solve by inner-hierarchy PCG instead of a dense inverse
  // coarse solve by GMRES preconditioned by one V-cycle of an inner hierarchy of A_c (a coarse
  // operator that is not SPD and beyond the dense inverse's size: the reference's SuperLU
  // factors any nonsingular A_H, ns/lib/multigrid.py:165-170)
  mlamg_hier* gm_inner = nullptr;
  double gm_rtol = 1e-14, gm_fail_rtol = 1e-10;
  int gm_restart = 50, gm_maxiter = 20;
  int32_t gm_solves = 0, gm_last_iters = 0, gm_total_iters = 0, gm_not_converged = 0;
  double gm_worst_rel = 0.0;
  double* xc = nullptr;
  double* bc = nullptr;
  int nu_pre = 1, nu_post = 1;
  int norm_mode = 0;  // per-cycle history: 0 = ||b - A x||_2, 1 = ||x||_2 (amg_2_v error_tol)
  void* mem = nullptr;
  size_t mem_bytes = 0;
  double* partial = nullptr;
  int32_t* flags = nullptr;  // [0] counter, [1] done
  bool ready = false;
  // captured single cycle (mlamg_hier_vcycle), and captured zero-guess cycle with level 0 as a
  // coarse level (hier_coarse_cycle: a Krylov preconditioner, or the distributed executor's
  // replicated levels). Each is re-keyed on its own; a setter that changes the cycle drops both
  mlamg::CycleGraph top_graph, coarse_graph;
  void invalidate_graphs() {
    top_graph.invalidate();
    coarse_graph.invalidate();
  }
  mlamg::DoneHost done_host;  // pinned copy of flags[1], polled between batches of cycles
  // the stop flag the cycle's kernels test: flags + 1, or nullptr while a no-tolerance
  // mlamg_hier_vcycle runs (nothing can raise it, and every kernel would otherwise start with a
  // dependent load of it). done_check = 1 keeps it on every launch (A/B, mlamg_hier_set_done_check)
  int32_t* cur_done = nullptr;
  int done_check = 0;
  // a Krylov solver's workspace (gmres.hip), kept across calls and grown on demand: at C4 a
  // restart-100 GMRES needs 101 fine vectors (8 GB), too large for the allocation cache
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // zero right-hand side for the paths that read b as a vector (Gauss-Seidel, coarse-only)
  double* zero_b = nullptr;
  bool zero_rhs = false;  // the last mlamg_hier_vcycle had b = NULL (cycle_bytes prices that)
  // k-wide copies of the level vectors for mlamg_hier_vcycle_mv, grown on demand
  void* mv_mem = nullptr;
  size_t mv_bytes = 0;
  // mlamg_hier_vcycle_mv takes Gauss-Seidel levels (mlamg_hier_set_mv_gauss_seidel)
  bool mv_gs = false;
  // mlamg_hier_vcycle_mv takes VECTOR-format operators (mlamg_hier_set_mv_vector)
  bool mv_vec = false;
};

namespace mlamg {
// Hands out consecutive 256-byte-aligned blocks of doubles from `base`. With base = nullptr it
// only measures, so one layout function, run first on nullptr and then on the allocation, both
// sizes a work buffer and carves it: the two passes cannot get out of step.
struct Carver {
  char* base;
  size_t off = 0;
  char* here() const { return base ? base + off : nullptr; }
  double* take(int64_t n) {
    double* q = reinterpret_cast<double*>(here());
    off += (sizeof(double) * (size_t)std::max<int64_t>(n, 1) + 255) & ~size_t(255);
    return q;
  }
};

// rows of the coarsest operator, whichever solver holds it (hier.hip)
int64_t coarse_rows(const mlamg_hier* H);
// allocate and carve H->mem on first use; EINVAL without a coarse solver (hier.hip)
int hier_prepare(mlamg_hier* H);
}  // namespace mlamg
