// Segmented per-column norm and mean removal of a stacked multivector (include/mlamg.h
// mlamg_norm2_seg_mv, mlamg_remove_mean_seg_mv): the rows of an n x k block are cut into nb
// consecutive segments (one per problem of a block-diagonal batch, mlamg/loss.py AmgLossBatch) and
// every segment is reduced on its own, all segments in one launch per stage.
//
// Parity: segment s keeps the partition of the single kernels of spmm.hip on its rows alone.
//   norm  k_colsum_partial<true> on nbs = min(1024, max(1, ceil(n_s / 256))) row blocks, block b
//         walking the rows b*256 + t + m*nbs*256; k_colsum_sqrt over the nbs partials;
//   mean  k_colsum_partial<false> on the fixed 512 row blocks; k_coltotal over the 512 partials;
//         k_colsub_mean dividing by n_s.
// The launch grid is sized by the longest segment: blockIdx.x runs over G = min(cap, ceil(max_len /
// 256)) row blocks. A norm block beyond a segment's nbs does not exist in the single launch and
// returns. A mean block that owns no rows writes the +0.0 the single kernel computes there, and the
// blocks G..511, which own no rows in any segment, are not launched: the total adds +0.0 in their
// position. So every segment's result is bitwise the single call on that segment's rows.
#include "common.hpp"
#include "reduce.hpp"

namespace mlamg {

namespace {

// k_colsum_partial of segment blockIdx.z on the columns [8 blockIdx.y, 8 blockIdx.y + 8);
// partial[((seg * k + col) * G) + b], G = gridDim.x
template <bool SQ>
__global__ __launch_bounds__(256) void k_seg_colsum_partial(const double* __restrict__ X,
                                                            int64_t ldx, int k,
                                                            const int64_t* __restrict__ off,
                                                            double* __restrict__ partial) {
  __shared__ double red[4][kColTile];
  const int seg = blockIdx.z;
  const int64_t r0 = off[seg], ns = off[seg + 1] - r0;
  const int G = gridDim.x;
  const int nbs = SQ ? min(reduce_grid(ns, 256, kNormGridCap), G) : kSumGrid;
  if ((int)blockIdx.x >= nbs) return;
  const int c0 = blockIdx.y * kColTile;
  const int nc = min(kColTile, k - c0);
  double* out = partial + ((int64_t)seg * k + c0) * G + blockIdx.x;
  if constexpr (!SQ) {
    if (blockIdx.x * 256ll >= ns) {
      // no rows: the sum the single kernel's block computes from its zero accumulators
      if ((int)threadIdx.x < nc) out[(int64_t)threadIdx.x * G] = 0.0;
      return;
    }
  }
  double acc[kColTile];
#pragma unroll
  for (int c = 0; c < kColTile; ++c) acc[c] = 0.0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < ns; i += (int64_t)nbs * 256) {
    const double* p = X + (r0 + i) * ldx + c0;
#pragma unroll
    for (int c = 0; c < kColTile; ++c) {
      if (c < nc) {
        const double v = p[c];
        if constexpr (SQ) {
          acc[c] += v * v;
        } else {
          acc[c] += v;
        }
      }
    }
  }
  const bool mine = (int)threadIdx.x < nc;
  const double t = tile_sum<256>(acc, red, mine);
  if (mine) out[(int64_t)threadIdx.x * G] = t;
}

// k_colsum_sqrt of (column blockIdx.x, segment blockIdx.y)
__global__ __launch_bounds__(1024) void k_seg_colsum_sqrt(const double* __restrict__ partial,
                                                          int G, int k,
                                                          const int64_t* __restrict__ off,
                                                          double* __restrict__ out) {
  __shared__ double red[16];
  const int seg = blockIdx.y;
  const int nbs = min(reduce_grid(off[seg + 1] - off[seg], 256, kNormGridCap), G);
  const double* p = partial + ((int64_t)seg * k + blockIdx.x) * G;
  const double t = partials_total<1024>(p, nbs, red);
  if (threadIdx.x == 0) out[(int64_t)seg * k + blockIdx.x] = sqrt(t);
}

// k_coltotal of (column blockIdx.x, segment blockIdx.y): thread t adds partials t and t + 256 of
// the 512 in that order (strided_sum's tail loop); a block that was not launched contributes +0.0
__global__ __launch_bounds__(256) void k_seg_coltotal(const double* __restrict__ partial, int G,
                                                      int k, double* __restrict__ out) {
  __shared__ double red[4];
  const int seg = blockIdx.y;
  const double* p = partial + ((int64_t)seg * k + blockIdx.x) * G;
  double s = 0.0;
  for (int i = threadIdx.x; i < kSumGrid; i += 256) s += i < G ? p[i] : 0.0;
  s = block_sum<256>(s, red);
  if (threadIdx.x == 0) out[(int64_t)seg * k + blockIdx.x] = s;
}

// k_colsub_mean of segment blockIdx.y
__global__ __launch_bounds__(256) void k_seg_colsub_mean(double* __restrict__ X, int64_t ldx,
                                                         int k, const int64_t* __restrict__ off,
                                                         const double* __restrict__ sum) {
  const int seg = blockIdx.y;
  const int64_t r0 = off[seg], ns = off[seg + 1] - r0;
  const int64_t w = blockIdx.x * 256ll + threadIdx.x;
  if (w >= ns * k) return;
  const int64_t i = w / k;
  const int c = (int)(w - i * k);
  const double mean = sum[(int64_t)seg * k + c] / (double)ns;
  X[(r0 + i) * ldx + c] = X[(r0 + i) * ldx + c] - mean;
}

constexpr int64_t kSegMaxSegments = 65535;  // a grid dimension

}  // namespace

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_norm2_seg_mv(const double* X, int64_t ldx, int k, const int64_t* seg_offsets,
                       int64_t nb, int64_t max_len, double* out, void* stream) {
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(seg_offsets, "seg_offsets is NULL");
  MLAMG_REQUIRE(out, "out is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(nb >= 1 && nb <= kSegMaxSegments, "nb must be in [1, 65535]");
  MLAMG_REQUIRE(max_len >= 0, "max_len < 0");
  hipStream_t s = S(stream);
  const int G = reduce_grid(max_len, 256, kNormGridCap);
  double* partial =
      static_cast<double*>(scratch(sizeof(double) * (size_t)nb * (size_t)k * (size_t)G, 17));
  MLAMG_REQUIRE(partial, "scratch allocation failed");
  hipLaunchKernelGGL(k_seg_colsum_partial<true>,
                     dim3(G, (k + kColTile - 1) / kColTile, (unsigned)nb), dim3(256), 0, s, X, ldx, k,
                     seg_offsets, partial);
  hipLaunchKernelGGL(k_seg_colsum_sqrt, dim3(k, (unsigned)nb), dim3(1024), 0, s, partial, G, k,
                     seg_offsets, out);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_remove_mean_seg_mv(double* X, int64_t ldx, int k, const int64_t* seg_offsets,
                             int64_t nb, int64_t max_len, void* stream) {
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(seg_offsets, "seg_offsets is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(nb >= 1 && nb <= kSegMaxSegments, "nb must be in [1, 65535]");
  MLAMG_REQUIRE(max_len >= 0, "max_len < 0");
  if (max_len == 0) return MLAMG_OK;
  hipStream_t s = S(stream);
  const int G = reduce_grid(max_len, 256, kSumGrid);  // max_len >= 1 here
  double* partial = static_cast<double*>(
      scratch(sizeof(double) * (size_t)nb * (size_t)k * (size_t)(G + 1), 18));
  MLAMG_REQUIRE(partial, "scratch allocation failed");
  double* total = partial + (size_t)nb * (size_t)k * (size_t)G;
  hipLaunchKernelGGL(k_seg_colsum_partial<false>,
                     dim3(G, (k + kColTile - 1) / kColTile, (unsigned)nb), dim3(256), 0, s, X, ldx, k,
                     seg_offsets, partial);
  hipLaunchKernelGGL(k_seg_coltotal, dim3(k, (unsigned)nb), dim3(256), 0, s, partial, G, k, total);
  hipLaunchKernelGGL(k_seg_colsub_mean, dim3((unsigned)((max_len * k + 255) / 256), (unsigned)nb),
                     dim3(256), 0, s, X, ldx, k, seg_offsets, total);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

}  // extern "C"
