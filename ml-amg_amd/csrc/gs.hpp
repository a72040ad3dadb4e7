// The Gauss-Seidel handle and the row arithmetic shared by the single-vector sweeps (gs.hip) and
// the block sweep (gs_mv.hip).
#pragma once
#include "common.hpp"

struct mlamg_gs {
  const mlamg_csr* A = nullptr;
  bool block = false;        // block_gauss_seidel arithmetic (pk_diag then holds Dinv)
  bool backward = false;     // rows swept n-1..0
  mlamg_gs* bwd = nullptr;   // symmetric sweep: the backward schedule of the same operator
  int32_t n_levels = 0;
  int32_t max_level_rows = 0;
  std::vector<int32_t> level_ptr;  // host
  int32_t* d_level_ptr = nullptr;  // device copy
  int32_t* rows = nullptr;         // device, rows grouped by level (ascending within a level)
  // level-ordered copy for the pipelined one-workgroup sweep (k_gs_pipe): position p = the p-th
  // row of `rows`; its off-diagonal entries in stored order in slots pk_col/pk_val[p*K .. p*K+K)
  // (column -1 pads), its diagonal (the last stored one, as the sequential sweep takes it; 0.0
  // when absent) in pk_diag[p]; b_lvl[p] = b[rows[p]] is refreshed per sweep. Every load of a
  // level's structure is then independent of the others. Snapshot of A at mlamg_gs_create.
  int32_t pk_k = 0;  // slots per row (4 or 8), 0 = no packed copy
  int32_t* pk_col = nullptr;
  double* pk_val = nullptr;
  double* pk_diag = nullptr;
  double* b_lvl = nullptr;
  int32_t max_off = 0;  // longest off-diagonal count
  // level-ordered (row, first entry, length, 0) per position for the wave-cooperative sweep
  // (rows with more than 8 off-diagonals, at most 128 entries per row; nullptr: none)
  int32_t* wpos = nullptr;
  int32_t max_len = 0;
  // ring sweep (k_gs_ring): slot columns classified earlier (ring position) / later (-(c + 2))
  int32_t* rcol = nullptr;
  double* rpv = nullptr;  // per slot: a, the later-swept product, or 0 (k_gs_ring_prep)
  uint16_t* rcode = nullptr;  // per slot: ring slot / kGsRingLater / kGsRingPad
  // the long-row ring sweep (k_gs_wring): SPAN slots per position, step table, ring
  int32_t wr_lpr = 0, wr_epl = 0, wr_steps = 0, wr_log2 = 0;
  int32_t* wr_code = nullptr;
  double* wr_pv = nullptr;
  int32_t* wr_len = nullptr;
  double* wr_d = nullptr;
  int2* wr_st = nullptr;
  size_t wr_lds = 0;
  double* rxl = nullptr;      // the sweep's values in level order
  int32_t ring_log2_r = 0;
  // windowed one-wave sweep (k_gs_win): x by level-order position in an LDS ring of 2^ring_log2
  // slots; wcol = the packed columns as positions (pads -1); chunks of levels staged into two
  // LDS buffers of win_cap + 1 positions; win_w = the widest level distance of a coupling
  int32_t win_rw = 0;  // 64-row slots per level (0: no windowed sweep)
  int32_t ring_log2 = 0, win_cap = 0, win_w = 0, n_chunks = 0;
  int32_t* wcol = nullptr;
  int32_t* d_clev = nullptr;  // the chunk plan (8 ints per chunk) + level starts
  double* win_xl = nullptr;  // x in level order (the window's old-x source)
  size_t win_lds = 0;
};

namespace mlamg {

// the two row updates: gauss_seidel (BLK false) sums the off-diagonal products from +0.0 and
// divides b_i minus the sum by the diagonal; block_gauss_seidel (BLK true) subtracts each product
// (gemm's 0 + a x) from b_i and multiplies by Dinv_i (gemm's 0 + d r)
template <bool BLK>
__device__ __forceinline__ double gs_init(double bi) { return BLK ? bi : 0.0; }
template <bool BLK>
__device__ __forceinline__ double gs_acc(double s, double a, double xj) {
  return BLK ? s - (0.0 + a * xj) : s + a * xj;
}
// d: the diagonal (gauss_seidel) or Dinv (block)
template <bool BLK>
__device__ __forceinline__ double gs_fin(double s, double bi, double d) {
  return BLK ? 0.0 + d * s : (bi - s) / d;
}
// gauss_seidel leaves a zero-diagonal row alone; block_gauss_seidel updates every row
template <bool BLK>
__device__ __forceinline__ bool gs_upd(double d) { return BLK || d != 0.0; }

// one workgroup of the whole-sweep kernels
constexpr int kGsBlock = 1024;

}  // namespace mlamg
