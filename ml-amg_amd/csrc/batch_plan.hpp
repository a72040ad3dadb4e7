// What the kernels of batch.hip and the host planner of batch_plan.cpp must agree on, written
// once: the batched solver's limits, the problem descriptor the kernels read, and the LDS-size
// formulas of the kernels' carves. Host-only: standard headers and the C-ABI, no HIP — the planner
// builds and runs (and is tested, tests/test_batch_plan_host.py) without a GPU toolchain.
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mlamg.h"

namespace mlamg {

constexpr int kBT = 1024;           // threads of a problem's workgroup
constexpr int64_t kBMaxN = 16384;   // fine rows: x lives in LDS during the cycles
constexpr int64_t kBMaxNc = 2048;   // coarse rows: dense inverse, LDS panels of >= 4 columns
constexpr int kBMaxK = 32;          // off-diagonal entries per row of A
constexpr int kBMaxKP = 32;         // entries per row of P
constexpr int kBMaxKT = 256;        // entries per row of P^T
constexpr int kBMaxPanel = 16;
constexpr int kExtCoarseMin = 300;  // single calls above this n_c: device-wide coarse factor
constexpr size_t kBLdsBytes = 156 * 1024;
constexpr int kBandMax = 63;  // half-bandwidth limit: rows (j, j + b] within the 64 lanes
// coarse size limit: the substitutions run on one wave, ~45 ns per row and direction; a single
// call with a larger coarse operator is faster with the device-wide dense factor and its coarse
// solve spread over the CUs (128^2: 13 vs 26 ms). Every batch-eligible size (n_c <= 1024, the
// Python engine's FUSED_BATCH_MAX_NC) is below it, so batches and single calls choose alike.
constexpr int kBandMaxNc = 1024;
constexpr int kBandPad = 32;  // zero steps before and after the band solve's lane layout

struct BDesc {
  int32_t n, nc, smoother, nu_pre, nu_post, norm_mode, max_iter;
  int32_t K, KA, KP, KT, nlev, panel, n_chunks, cap, timing;
  int32_t spd;    // A symmetric: try the inverse Cholesky factor before Gauss-Jordan
  int32_t chol_nb;  // its panel width (4..16, from n_c)
  int32_t setup_mode;  // 0: Galerkin + coarse inverse here; 1: neither (k_galerkin_rows and the
                       // device-wide factorisation of dense.hip); 2: Galerkin only (the batched
                       // device-wide factorisation follows); 3: nothing (a relaunch's bystander)
  int32_t gs_rw;  // one-wave sweep (rows of K = 4 or 8 slots, levels <= 64 * gs_rw rows), 1 or 2
                  // rows per lane; 0: the workgroup sweeps each level
  int32_t gs_db;   // one-wave sweep: double-buffered chunk staging (chunks of >= 3 levels)
  int32_t gs_rp;   // one-wave sweep, one buffer: the next chunk prefetched into registers
  int32_t phased;  // single large problem: each cycle is two launches, the workgroup's half
                   // cycles and the coarse solve on every CU (k_amg2v_coarse); r_H, e_H global
  double tol, omega;
  // byte offsets into the arena; packed arrays are slot-major: a[s * rows + row]
  int64_t ak_col, ak_val;                  // A rows, stored order incl. diagonal (KA slots)
  int64_t pp_col, pp_val;                  // P rows (KP slots)
  int64_t pt_row, pt_val;                  // P^T rows: fine rows ascending (KT slots)
  int64_t lev_ptr, chunk_lev, pk_row, pk_col, pk_val, pk_diag, b_lvl;  // sweep, level order
  int64_t b, x0;
  int64_t AH, AI, rg, dinv;                // Galerkin / un-pivoted inverse / r when not in
                                           // LDS / weighted-Jacobi weights
  int64_t x_out, err_out, stat_out;
  int64_t rcg, eg, yg;  // phased: r_H, e_H and L^-1 r_H in the arena
  int64_t done_ctr;     // phased: problems finished (one counter for the launch)
  // the problem's values as the caller stores them (A.data, P.data) and its shape's gather maps
  // (shared by every problem with the same sparsity): the packed value arrays above are
  // gathered from them on the device (gather_values), so only the caller's values travel
  int64_t a_raw, p_raw;
  int64_t a_map, p_map, t_map, g_map, d_map, pk_row0;
  // banded coarse solve (band_ld = half-bandwidth + 1, 0: dense): the factor in the band
  // solve's lane layouts F (forward) and G (backward), reciprocal diagonal
  int32_t band_ld, pad0;
  int64_t lc, lr, rinv;
};
static_assert(sizeof(BDesc) == 416, "BDesc is read by the kernels: field order and padding fixed");

// ---- LDS bytes of the kernels' dynamic carves (the planner sizes launches and chunks with them)
// chol_inverse: two NB x (NB + 1) blocks, the L21 panel and the Z rows
inline size_t chol_lds(int nb, int64_t nc) {
  return (size_t)8 * (2 * nb * (nb + 1) + (size_t)nc * (nb + 1) + (size_t)nb * nc);
}
// band_chol's rings: w x (w + 1) window, w diagonals
inline size_t band_lds(int b) {
  size_t w = 1;
  while (w < (size_t)b + 2) w <<= 1;
  return 8 * (w * (w + 1) + w);
}
// k_amg2v_setup's Gauss-Jordan: the n_c x (b + 1) panel, pivots, permutation
inline size_t gj_lds(int b, int64_t nc) { return (size_t)nc * (b + 1) * 8 + 16 * b + (size_t)nc * 12; }
// k_amg2v_cycles' vectors (xs, rs, rcs, es): x (+ zero and sink slots), r when it fits (L^-1 r_H shares it), and,
// unless phased (then they live in the arena), r_H and e_H
inline size_t cycle_vec_lds(int64_t n, int64_t nc, bool r_lds, bool phased) {
  return (size_t)n * 8 * (r_lds ? 2 : 1) + 16 + (phased ? 0 : (size_t)nc * 16);
}
// k_amg2v_cycles' sweep staging (stage): per position K columns, K values, diagonal, b, row; one or
// (gs_db) two buffers
inline size_t stage_pos_lds(int K, bool db) { return (12 * (size_t)K + 24) * (db ? 2 : 1); }
// k_amg2v_cycles' whole carve for a staging capacity of cap positions (+ the dummy position)
inline size_t cycles_lds(size_t vec_lds, int cap, int K, bool db) {
  return vec_lds + 16 + (size_t)(cap + 1) * stage_pos_lds(K, db) + 40;
}

struct Shape;  // a pattern's packed structure for one set of batch flags (batch_plan.cpp)

struct BatchPlan {            // everything mlamg_amg2v_batch needs after planning
  std::vector<BDesc> desc;    // filled, offsets final
  std::vector<int32_t> cblk;  // phased: first coarse-solve block per problem
  int64_t desc_off = 0, cblk_off = 0, done_off = 0;
  size_t in_bytes = 0, out_begin = 0, total = 0;
  size_t lds_setup = 0, lds_cycles = 0, lds_band = 0;
  bool phased = false, r_lds = false, any_band = false, ext_coarse = false, batch_ext = false,
       two_pass = false, rp = false;
  bool timing = false;  // MLAMG_BATCH_TIMING: the kernels stamp phases, the entry prints them
  std::chrono::steady_clock::time_point t_analysed;  // analysis done, layout begins
  // the distinct shapes and a problem that carries each one's arena offsets, for fill_inputs
  std::vector<std::shared_ptr<const Shape>> shapes;
  std::vector<int> shape_rep;
  int code = MLAMG_OK;
  std::string err;  // the refusal's message, "(problem q)" included
};

// Validates the problems, analyses their patterns (cached across calls), chooses the strategy and
// lays out the arena. Returns out->code; never touches the device or the library's error state.
int plan_batch(const mlamg_amg2v_problem* probs, int count, int smoother, int nu_pre, int nu_post,
               double jacobi_weight, int norm_mode, double tol, int max_iter, BatchPlan* out);
// the arena's input part [0, in_bytes) into host_buf: descriptors, shapes, the callers' values
void fill_inputs(const BatchPlan& plan, const mlamg_amg2v_problem* probs, char* host_buf);
// the arena's output part [out_begin, total), copied to host_out, into the problems
void read_outputs(const BatchPlan& plan, mlamg_amg2v_problem* probs, const char* host_out,
                  int max_iter);

}  // namespace mlamg
