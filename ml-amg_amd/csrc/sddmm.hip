// Sampled dense-dense product on a CSR pattern (include/mlamg.h mlamg_sddmm):
//   out[e] = alpha * sum_{c<k} U[row(e), c] * V[col(e), c] + beta * out[e]
// for every stored entry e of S, in S's CSR entry order. The gradient of amg_loss with respect to
// the prolongator's stored values is two of these per cycle (mlamg/loss.py).
//
// SUMMATION ORDER (part of the contract; tests/test_gpu_sddmm.py restates it in numpy). With
// G = the smallest power of two >= ceil(k / 2) (1 <= G <= 32) and U[i, c] = V[j, c] = +0.0 for
// k <= c < 2 G:
//   t[p]  = (U[i, 2p] * V[j, 2p]) + (U[i, 2p+1] * V[j, 2p+1])            p = 0 .. G-1
//   then, while more than one term is left:  t[q] = t[2q] + t[2q+1]       q = 0 .. len/2 - 1
//   s     = t[0]
//   out   = alpha * s                    (beta == 0: out is not read)
//   out   = (alpha * s) + (beta * out)   (otherwise)
// Every multiply and add rounds on its own (-ffp-contract=off). The sum of an entry is a function
// of k, U[i, :] and V[j, :] alone: not of the row-block partition, the entry's place in its row,
// the leading dimensions, the alignment of the pointers or the instantiation that ran.
//
// Shape: k_spmm_stream's. One 256-thread workgroup per row block of the handle's table (<= 256
// rows, <= 2048 nonzeros, or one over-long row) stages the block's column indices in LDS with
// coalesced non-temporal loads. A group of G adjacent lanes owns a row: lane p keeps
// U[i, 2p : 2p+2] in registers for the whole row, and for each entry loads V[j, 2p : 2p+2] as one
// 16-byte piece, so every global access of a group is one contiguous k * 8-byte run. The group
// adds its G terms with an xor butterfly over the lane distances 1, 2, 4, 8, 16 (the pairwise tree
// above: both partners add the same two values, so every lane of the group ends with the same
// bits). Entries are taken four at a time (four gathers in flight per lane); lanes 0..3 of the
// group store one result each (G < 4: lane q mod G). An over-long row's entries are dealt over
// the 256 / G groups of its workgroup, four adjacent entries at a time.
// The 16-byte accesses need 16-byte aligned U and V and even leading dimensions (VEC); otherwise
// the same kernel runs with 8-byte accesses.
#include "common.hpp"

#include <hip/hip_runtime.h>

namespace mlamg {

__device__ __forceinline__ int64_t xcd_block_sd(int64_t b, int64_t nb) {
  const int64_t q = nb >> 3, r = nb & 7, g = b & 7, i = b >> 3;
  return (g < r ? g * (q + 1) : r * (q + 1) + (g - r) * q) + i;
}

// columns (c, c + 1) of a multivector row at p: nothing is read of a column >= k
template <bool VEC>
__device__ __forceinline__ void ld_pair(const double* __restrict__ p, bool has, bool two, double& a,
                                        double& b) {
  a = 0.0;
  b = 0.0;
  if (!has) return;
  if constexpr (VEC) {
    if (two) {
      const double2 t = *reinterpret_cast<const double2*>(p);
      a = t.x;
      b = t.y;
    } else {
      a = p[0];
    }
  } else {
    a = p[0];
    if (two) b = p[1];
  }
}

// the value of lane (lane ^ OFF): distances 1 and 2 are quad permutes and 8 a rotation of the row
// of 16 (DPP, no LDS traffic); 4 and 16 go through the swizzle unit (bit-mask mode, xor mask OFF)
template <int OFF>
__device__ __forceinline__ int xor_lane_i32(int v) {
  if constexpr (OFF == 1) {
    return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);  // quad_perm:[1,0,3,2]
  } else if constexpr (OFF == 2) {
    return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);  // quad_perm:[2,3,0,1]
  } else if constexpr (OFF == 8) {
    return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);  // row_ror:8
  } else {
    return __builtin_amdgcn_ds_swizzle(v, (OFF << 10) | 0x1F);
  }
}

template <int OFF>
__device__ __forceinline__ double xor_lane(double v) {
  const int lo = xor_lane_i32<OFF>(__double2loint(v));
  const int hi = xor_lane_i32<OFF>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// the pairwise tree over the G lanes of a group; every lane returns the group's sum
template <int G>
__device__ __forceinline__ double group_sum(double t) {
  if constexpr (G >= 2) t = t + xor_lane<1>(t);
  if constexpr (G >= 4) t = t + xor_lane<2>(t);
  if constexpr (G >= 8) t = t + xor_lane<4>(t);
  if constexpr (G >= 16) t = t + xor_lane<8>(t);
  if constexpr (G >= 32) t = t + xor_lane<16>(t);
  return t;
}

__device__ __forceinline__ void sddmm_store(double* __restrict__ o, double s, double alpha,
                                            double beta) {
  if (beta == 0.0) {
    *o = alpha * s;
  } else {
    const double a = alpha * s;
    const double b = beta * *o;
    *o = a + b;
  }
}

// Entries [ea, eb) of one row in bundles of four, a bundle every `step` entries: col[e] is the
// column of entry e and out[e] its result. All G lanes of the group run this with the same
// arguments but p (the butterfly needs the whole group in step).
template <int G, bool VEC>
__device__ __forceinline__ void sddmm_entries(const int32_t* col, int ea, int eb, int step, int p,
                                              bool has, bool two, double u0, double u1,
                                              const double* __restrict__ Vc, int64_t ldv,
                                              double alpha, double beta, double* __restrict__ out) {
  for (int e = ea; e < eb; e += step) {
    double v0[4], v1[4], s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool live = e + q < eb;
      const int64_t j = live ? col[e + q] : 0;
      ld_pair<VEC>(Vc + j * ldv, has && live, two, v0[q], v1[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double a = u0 * v0[q];
      const double b = u1 * v1[q];
      s[q] = group_sum<G>(a + b);
    }
    if constexpr (G >= 4) {
      const double mine = p == 0 ? s[0] : (p == 1 ? s[1] : (p == 2 ? s[2] : s[3]));
      if (p < 4 && e + p < eb) sddmm_store(out + e + p, mine, alpha, beta);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((q & (G - 1)) == p && e + q < eb) sddmm_store(out + e + q, s[q], alpha, beta);
    }
  }
}

template <int G, bool VEC>
__global__ __launch_bounds__(kThreads) void k_sddmm(const int32_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const int32_t* __restrict__ blk,
                                                    const double* __restrict__ U, int64_t ldu,
                                                    const double* __restrict__ V, int64_t ldv, int k,
                                                    double alpha, double beta,
                                                    double* __restrict__ out) {
  __shared__ int32_t sc[kBlockNnz];
  __shared__ int32_t rp[kBlockRows + 1];
  constexpr int NG = kThreads / G;  // groups (rows in flight) per workgroup
  const int b = (int)xcd_block_sd(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  const int r0 = blk[b];
  const int r1 = blk[b + 1];
  const int nr = r1 - r0;
  const int e0 = indptr[r0];
  const int ne = indptr[r1] - e0;
  const int p = tid & (G - 1);
  const int g = tid / G;
  const int c = p << 1;
  const bool has = c < k;
  const bool two = c + 1 < k;
  const double* Vc = V + c;
  double* oe = out + e0;
  if (ne <= kBlockNnz) {
    const int32_t* ci = indices + e0;
    constexpr int UN = kBlockNnz / kThreads;
    int32_t cc[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int e = tid + u * kThreads;
      cc[u] = e < ne ? __builtin_nontemporal_load(ci + e) : 0;
    }
    for (int t = tid; t <= nr; t += kThreads) rp[t] = indptr[r0 + t] - e0;
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int e = tid + u * kThreads;
      if (e < ne) sc[e] = cc[u];
    }
    __syncthreads();
    for (int t = g; t < nr; t += NG) {
      const int ka = rp[t], kb = rp[t + 1];
      if (ka == kb) continue;
      double u0, u1;
      ld_pair<VEC>(U + (int64_t)(r0 + t) * ldu + c, has, two, u0, u1);
      sddmm_entries<G, VEC>(sc, ka, kb, 4, p, has, two, u0, u1, Vc, ldv, alpha, beta, oe);
    }
  } else {
    // one over-long row: its entries dealt over the groups, the columns read from global memory
    double u0, u1;
    ld_pair<VEC>(U + (int64_t)r0 * ldu + c, has, two, u0, u1);
    sddmm_entries<G, VEC>(indices + e0, g * 4, ne, NG * 4, p, has, two, u0, u1, Vc, ldv, alpha,
                          beta, oe);
  }
}

static inline bool al16_sd(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int G>
static void launch_sddmm_g(const mlamg_csr* S, const double* U, int64_t ldu, const double* V,
                           int64_t ldv, int k, double alpha, double beta, double* out, bool vec,
                           hipStream_t s) {
  if (vec) {
    MLAMG_LAUNCH((k_sddmm<G, true>), dim3(S->n_blocks), dim3(kThreads), 0, s, S->indptr,
                 S->indices, S->blk, U, ldu, V, ldv, k, alpha, beta, out);
  } else {
    MLAMG_LAUNCH((k_sddmm<G, false>), dim3(S->n_blocks), dim3(kThreads), 0, s, S->indptr,
                 S->indices, S->blk, U, ldu, V, ldv, k, alpha, beta, out);
  }
}

int sddmm_impl(const mlamg_csr* S, const double* U, int64_t ldu, const double* V, int64_t ldv,
               int k, double alpha, double beta, double* out, hipStream_t s) {
  if (S->n_rows == 0 || S->nnz == 0 || S->n_blocks == 0) return MLAMG_OK;
  MLAMG_REQUIRE(S->blk != nullptr, "pattern has no row-block table");
  const bool vec = al16_sd(U) && !(ldu & 1) && al16_sd(V) && !(ldv & 1);
  const int half = (k + 1) >> 1;
  if (half <= 1) {
    launch_sddmm_g<1>(S, U, ldu, V, ldv, k, alpha, beta, out, vec, s);
  } else if (half <= 2) {
    launch_sddmm_g<2>(S, U, ldu, V, ldv, k, alpha, beta, out, vec, s);
  } else if (half <= 4) {
    launch_sddmm_g<4>(S, U, ldu, V, ldv, k, alpha, beta, out, vec, s);
  } else if (half <= 8) {
    launch_sddmm_g<8>(S, U, ldu, V, ldv, k, alpha, beta, out, vec, s);
  } else if (half <= 16) {
    launch_sddmm_g<16>(S, U, ldu, V, ldv, k, alpha, beta, out, vec, s);
  } else {
    launch_sddmm_g<32>(S, U, ldu, V, ldv, k, alpha, beta, out, vec, s);
  }
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_sddmm(const mlamg_csr* S, const double* U, int64_t ldu, const double* V, int64_t ldv,
                int k, double alpha, double beta, double* out, void* stream) {
  MLAMG_REQUIRE(S, "S is NULL");
  MLAMG_REQUIRE(U, "U is NULL");
  MLAMG_REQUIRE(V, "V is NULL");
  MLAMG_REQUIRE(out, "out is NULL");
  MLAMG_REQUIRE(k >= 1 && k <= MLAMG_MV_MAX, "k must be in [1, MLAMG_MV_MAX = 64]");
  MLAMG_REQUIRE(ldu >= k, "ldu < k");
  MLAMG_REQUIRE(ldv >= k, "ldv < k");
  return sddmm_impl(S, U, ldu, V, ldv, k, alpha, beta, out, mlamg::S(stream));
}

}  // extern "C"
