// The Gauss-Seidel handle and the row arithmetic shared by the single-vector sweeps (gs.hip) and
// the block sweep (gs_mv.hip).
#pragma once
#include "common.hpp"
#include "gs_plan.hpp"

// A sweep direction's plan (gs_plan.hpp: its scalars, path included, are the base) and the device
// side of it. Snapshot of A at mlamg_gs_create.
struct mlamg_gs : mlamg::GsScalars {
  const mlamg_csr* A = nullptr;
  bool block = false;        // block_gauss_seidel arithmetic (pk_diag then holds Dinv)
  mlamg_gs* bwd = nullptr;   // symmetric sweep: the backward schedule of the same operator
  // every device buffer below, by the address of its field: gs_upload appends, destroy frees
  std::vector<void**> owned;
  std::vector<int32_t> level_ptr;  // host
  int32_t* d_level_ptr = nullptr;  // device copy
  int32_t* rows = nullptr;         // rows grouped by level (ascending within a level)
  // level-ordered packed copy (k_gs_pipe, k_gs_lds, k_gs_win, k_gs_ring; gs_mv.hip's walk):
  // position p's off-diagonal entries in stored order in slots [p*K, p*K+K) of pk_col / pk_val
  // (column -1 pads), its diagonal (the last stored one; 0.0 when absent) in pk_diag[p];
  // b_lvl[p] = b[rows[p]] is refreshed per sweep
  int32_t pk_k = 0;  // slots per row (4 or 8), 0 = no packed copy on the device
  int32_t* pk_col = nullptr;
  double* pk_val = nullptr;
  double* pk_diag = nullptr;
  double* b_lvl = nullptr;
  int32_t* wpos = nullptr;  // k_gs_wave: (row, first entry, length, 0) per position
  // k_gs_ring: slot columns classified earlier (ring position) / later (-(c + 2))
  int32_t* rcol = nullptr;
  double* rpv = nullptr;  // per slot: a, the later-swept product, or 0 (k_gs_ring_prep)
  uint16_t* rcode = nullptr;  // per slot: ring slot / kGsRingLater / kGsRingPad
  // k_gs_wring: SPAN slots per position, step table
  int32_t* wr_code = nullptr;
  double* wr_pv = nullptr;
  int32_t* wr_len = nullptr;
  double* wr_d = nullptr;
  int2* wr_st = nullptr;
  double* rxl = nullptr;      // the ring sweeps' values in level order
  // k_gs_win: wcol = the packed columns as positions (pads -1)
  int32_t* wcol = nullptr;
  int32_t* d_clev = nullptr;  // the chunk plan (8 ints per chunk) + level starts
  double* win_xl = nullptr;  // x in level order (the window's old-x source)
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

}  // namespace mlamg
