// Multi-vector (n x k) SpMM in the canonical CSR-vector order: per column the bits
// of the single-vector path with the VECTOR format active on the handle, at any width.
//
// The order is the one written down above k_csr_vcan (spmv.hip) and restated in oracle.c
// vec_matvec: virtual lane v = 64 w + l (w = 0..7, l = 0..63) sums the row's entries v, v + 512,
// ... left to right from +0.0 with separate multiply and add, skipping the entries it does not
// have; each virtual wave folds its 64 lane sums with the xor butterfly off = 32 .. 1; the row is
// ((ws_0 + ws_1) + ...) + ws_7. Only that addition tree is contractual: both partners of a
// butterfly step add the same two values, so any mapping that forms the same pairs gives the same
// bits.
//
// k_spmm_vcan: one 512-thread workgroup per row; physical wave w is virtual wave w. The columns
// are taken in tiles of kCT = 8 that loop inside the workgroup. Within a wave, lane l = 4 g + j
// (g = 0..15, j = 0..3) owns the column pair (2j, 2j + 1) of the tile for the four virtual lanes
// 4g .. 4g + 3: eight accumulators, as many as "thread = virtual lane, eight columns" needs, but
// the four lanes of a group read one entry's operand run X[col, c0 : c0 + 8] as four adjacent
// 16-byte pieces of one load instruction, which then touches 16 cache lines instead of 64 (the
// first version, thread = virtual lane with four 16-byte loads per entry, was bound by exactly
// that: DESIGN §22). A lane's four (column, value) entries of each 512-entry stripe stay in
// registers across the column tiles for a row of <= 1,024 entries, so the matrix stream is read
// once for all k columns; a longer row is re-read per tile (12 KiB or more that the workgroup has
// just pulled through its L2). Every load is unconditional with a clamped position (a branch join
// would drain the loads in flight): a slot without an entry re-reads the row's last
// one and a column pair past k re-reads one inside the block; neither is added to anything that
// is stored. The next tile's operands are requested before the current tile is folded.
//
// The fold (vc_wave_fold) forms the butterfly's pairs by recursive halving: the steps 32, 16, 8
// and 4 of the virtual lane number are steps 32, 16, 8 and 4 of the physical one (g's bits); after
// the first a lane keeps two of its four virtual lanes, after the second one, after the third one
// column of its pair; the steps 2 and 1 pair virtual lanes of one group, which by then sit in the
// lanes l ^ 32 and l ^ 16: 10 shuffles for 8 columns instead of 48. The eight wave sums per
// column go through LDS (two buffers, one barrier per tile); thread p < 4 adds them in order for
// the column pair (2p, 2p + 1) and applies the epilogue (spmm_epi.hpp).
#include "common.hpp"
#include "spmm_epi.hpp"

#include <hip/hip_runtime.h>

namespace mlamg {

constexpr int kCT = 8;         // columns per tile
constexpr int kVcLanes = 512;  // virtual lanes = threads per row
constexpr int kVcG = 4;        // virtual lanes (entries of a stripe) per physical lane

// how a lane reads its column pair: 8-byte loads; 16-byte loads (even k); 16-byte loads plus one
// 8-byte load for an odd k's last column (k >= 3)
enum VcMode : int { VC_8 = 0, VC_16 = 1, VC_16_ODD = 2 };

// entries base + 512 t + v0 + i of the row ending at b (> base); a slot past the end re-reads
// the row's last entry and is not live
template <int T, bool NT, typename IT>
__device__ __forceinline__ void vc_load(const IT* __restrict__ idx, const double* __restrict__ vals,
                                        int base, int b, int v0, int32_t (&cc)[T][kVcG],
                                        double (&vv)[T][kVcG], bool (&live)[T][kVcG]) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < kVcG; ++i) {
      const int e = base + kVcLanes * t + v0 + i;
      live[t][i] = e < b;
      const int ee = min(e, b - 1);
      if constexpr (NT) {
        cc[t][i] = (int32_t)__builtin_nontemporal_load(idx + ee);
        vv[t][i] = __builtin_nontemporal_load(vals + ee);
      } else {
        cc[t][i] = (int32_t)idx[ee];
        vv[t][i] = vals[ee];
      }
    }
}

// x[t][i][.] = X[col of entry (t, i), c : c + 2] for the lane's column pair c = c0 + 2 j. A pair
// or column past k is replaced by one inside the block (its sums are never stored).
template <int T, int MODE>
__device__ __forceinline__ void vc_gather(const int32_t (&cc)[T][kVcG],
                                          const double* __restrict__ X, int64_t ldx, int c, int k,
                                          double (&x)[T][kVcG][2]) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < kVcG; ++i) {
      const double* xr = X + (int64_t)cc[t][i] * ldx;
      if constexpr (MODE == VC_8) {
        x[t][i][0] = xr[min(c, k - 1)];
        x[t][i][1] = xr[min(c + 1, k - 1)];
      } else {  // c is even and the block 16-byte aligned with an even leading dimension
        const double2 v = *reinterpret_cast<const double2*>(xr + (c + 1 < k ? c : 0));
        x[t][i][0] = v.x;
        x[t][i][1] = v.y;
        if constexpr (MODE == VC_16_ODD) {
          const double last = xr[k - 1];
          x[t][i][0] = (c == k - 1) ? last : v.x;
        }
      }
    }
}

template <int T>
__device__ __forceinline__ void vc_fma(const double (&vv)[T][kVcG], const bool (&live)[T][kVcG],
                                       const double (&x)[T][kVcG][2], double (&acc)[kVcG][2]) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < kVcG; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double s = acc[i][h] + vv[t][i] * x[t][i][h];
        acc[i][h] = live[t][i] ? s : acc[i][h];
      }
}

// The xor butterfly off = 32 .. 1 over the wave's 64 virtual lanes, for the tile's 8 columns.
// acc[i][h]: virtual lane 4 (lane >> 2) + i, column 2 (lane & 3) + h. Returns the wave sum of
// column 2 (lane & 3) + bit 3 of the lane number (the same value in the 8 lanes that share it).
__device__ __forceinline__ double vc_wave_fold(const double (&acc)[kVcG][2], int lane) {
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
  double q[2][2], d[2];
  // off = 32: virtual lanes 4g + i and 4(g ^ 8) + i; keep i = 2 h5 + {0, 1}
#pragma unroll
  for (int i0 = 0; i0 < 2; ++i0)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double send = h5 ? acc[i0][h] : acc[2 + i0][h];
      const double keep = h5 ? acc[2 + i0][h] : acc[i0][h];
      q[i0][h] = keep + __shfl_xor(send, 32, 64);
    }
  // off = 16: keep i = 2 h5 + h4
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double send = h4 ? q[0][h] : q[1][h];
    const double keep = h4 ? q[1][h] : q[0][h];
    d[h] = keep + __shfl_xor(send, 16, 64);
  }
  // off = 8: keep column 2j + h3
  const double send = h3 ? d[0] : d[1];
  const double keep = h3 ? d[1] : d[0];
  double r = keep + __shfl_xor(send, 8, 64);
  r += __shfl_xor(r, 4, 64);   // off = 4
  r += __shfl_xor(r, 32, 64);  // off = 2: virtual lanes i and i ^ 2 sit in lanes l and l ^ 32
  r += __shfl_xor(r, 16, 64);  // off = 1: i and i ^ 1 in l and l ^ 16
  return r;
}

// the column tiles of one row. HELD: the row has at most 512 T entries, kept in registers
template <int T, bool HELD, int MODE, typename IT>
__device__ __forceinline__ void vc_row(const IT* __restrict__ idx, const double* __restrict__ vals,
                                       int a, int b, int64_t row, const double* __restrict__ X,
                                       int64_t ldx, int k, const EpiMV& ep,
                                       double (&ws)[2][8][kCT]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int v0 = 64 * wave + kVcG * (lane >> 2);  // the lane's first virtual lane
  const int cj = 2 * (lane & 3);                  // its column pair within a tile
  int32_t cc[T][kVcG];
  double vv[T][kVcG], x[T][kVcG][2];
  bool live[T][kVcG];
  const bool any = a < b;
  if constexpr (HELD) {
    if (any) {
      vc_load<T, true>(idx, vals, a, b, v0, cc, vv, live);
      vc_gather<T, MODE>(cc, X, ldx, cj, k, x);
    }
  }
  int buf = 0;
  for (int c0 = 0; c0 < k; c0 += kCT, buf ^= 1) {
    const int nc = min(kCT, k - c0);
    double acc[kVcG][2];
#pragma unroll
    for (int i = 0; i < kVcG; ++i) acc[i][0] = acc[i][1] = 0.0;
    if constexpr (HELD) {
      if (any) {
        vc_fma<T>(vv, live, x, acc);
        // the next tile's operands, in flight during the fold and the epilogue
        if (c0 + kCT < k) vc_gather<T, MODE>(cc, X, ldx, c0 + kCT + cj, k, x);
      }
    } else {
      for (int base = a; base < b; base += kVcLanes * T) {
        vc_load<T, false>(idx, vals, base, b, v0, cc, vv, live);
        vc_gather<T, MODE>(cc, X, ldx, c0 + cj, k, x);
        vc_fma<T>(vv, live, x, acc);
      }
    }
    const double r = vc_wave_fold(acc, lane);
    if ((lane & 0x34) == 0) ws[buf][wave][cj + ((lane >> 3) & 1)] = r;
    __syncthreads();
    // the other buffer is written only after the next barrier, which this thread joins after
    // its epilogue: one barrier per tile
    const int c = 2 * tid;
    if (c < nc) {
      double s0 = ws[buf][0][c], s1 = ws[buf][0][c + 1];
#pragma unroll
      for (int w = 1; w < 8; ++w) {
        s0 += ws[buf][w][c];
        s1 += ws[buf][w][c + 1];
      }
      epi_mv<MODE != VC_8>(row, c0 + c, c + 1 < nc, s0, s1, ep);
    }
  }
}

template <int MODE, typename IT>
__global__ __launch_bounds__(kVcLanes) void k_spmm_vcan(const int32_t* __restrict__ indptr,
                                                        const IT* __restrict__ idx,
                                                        const double* __restrict__ vals,
                                                        const double* __restrict__ X, int64_t ldx,
                                                        int k, EpiMV ep) {
  __shared__ double ws[2][8][kCT];
  if (ep.done && *ep.done) return;
  const int64_t row = blockIdx.x;
  const int a = indptr[row], b = indptr[row + 1];
  const int len = b - a;
  if (len <= kVcLanes) {
    vc_row<1, true, MODE>(idx, vals, a, b, row, X, ldx, k, ep, ws);
  } else if (len <= 2 * kVcLanes) {
    vc_row<2, true, MODE>(idx, vals, a, b, row, X, ldx, k, ep, ws);
  } else {
    vc_row<2, false, MODE>(idx, vals, a, b, row, X, ldx, k, ep, ws);
  }
}

template <int MODE>
static void launch_vcan_mode(const mlamg_csr* A, const double* X, int64_t ldx, int k,
                             const EpiMV& ep, hipStream_t s) {
  const dim3 grid((unsigned)A->n_rows), block(kVcLanes);
  if (A->vec_idx16)
    MLAMG_LAUNCH((k_spmm_vcan<MODE, uint16_t>), grid, block, 0, s, A->indptr, A->vec_idx16,
                 A->data, X, ldx, k, ep);
  else
    MLAMG_LAUNCH((k_spmm_vcan<MODE, int32_t>), grid, block, 0, s, A->indptr, A->indices, A->data,
                 X, ldx, k, ep);
}

int launch_spmm_vcan(const mlamg_csr* A, const double* X, int64_t ldx, int k, const EpiMV& ep,
                     hipStream_t s) {
  if (A->n_rows == 0) return MLAMG_OK;
  MLAMG_REQUIRE(A->n_rows <= 0x7fffffff, "more than 2^31 - 1 rows");
  // k == 1 has no column pair: 8-byte accesses
  if (k < 2 || !mv_vec16(X, ldx, ep))
    launch_vcan_mode<VC_8>(A, X, ldx, k, ep, s);
  else if (k & 1)
    launch_vcan_mode<VC_16_ODD>(A, X, ldx, k, ep, s);
  else
    launch_vcan_mode<VC_16>(A, X, ldx, k, ep, s);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_spmm_vec(const mlamg_csr* A, const double* X, int64_t ldx, double* Y, int64_t ldy,
                   int k, double alpha, double beta, void* stream) {
  MLAMG_REQUIRE(A, "A is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(Y, "Y is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(ldy >= k, "ldy < k");
  MLAMG_REQUIRE(X != Y, "X and Y must differ");
  return spmm_set_mv(A, X, ldx, Y, ldy, k, alpha, beta, S(stream), nullptr, true);
}

int mlamg_residual_mv_vec(const mlamg_csr* A, const double* B, int64_t ldb, const double* X,
                          int64_t ldx, double* R, int64_t ldr, int k, double* norms,
                          void* stream) {
  MLAMG_REQUIRE(A, "A is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(R, "R is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(ldr >= k, "ldr < k");
  MLAMG_REQUIRE(!B || ldb >= k, "ldb < k");
  MLAMG_REQUIRE(X != R, "X and R must differ");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "residual needs a square matrix");
  return residual_mv_run(A, B, ldb, X, ldx, R, ldr, k, norms, S(stream), true);
}

int mlamg_jacobi_mv_vec(const mlamg_csr* A, const double* dinv_w, const double* B, int64_t ldb,
                        double* X, int64_t ldx, double* X_tmp, int64_t ldt, int k, int nu,
                        void* stream) {
  MLAMG_REQUIRE(A, "A is NULL");
  MLAMG_REQUIRE(dinv_w, "dinv_w is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(X_tmp, "X_tmp is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(ldt >= k, "ldt < k");
  MLAMG_REQUIRE(!B || ldb >= k, "ldb < k");
  MLAMG_REQUIRE(nu >= 0, "nu < 0");
  MLAMG_REQUIRE(X != X_tmp, "X_tmp must differ from X");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "jacobi needs a square matrix");
  return jacobi_mv_run(A, dinv_w, B, ldb, X, ldx, X_tmp, ldt, k, nu, S(stream), true);
}

int mlamg_prolong_add_mv_vec(const mlamg_csr* P, const double* E, int64_t lde, double* X,
                             int64_t ldx, int k, void* stream) {
  MLAMG_REQUIRE(P, "P is NULL");
  MLAMG_REQUIRE(E, "E is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(lde >= k, "lde < k");
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  return spmm_add_mv(P, E, lde, X, ldx, k, S(stream), nullptr, true);
}

}  // extern "C"
