// Fixed-order reductions: the one statement of the order every norm, dot product and mean of the
// library is summed in. Results are deterministic, and the kernels whose results must be bitwise
// the same (column j of an _mv kernel and the single-vector kernel on column j; segment i of a
// _seg_mv kernel and the _mv kernel on that segment; column j of the block PCG and the single PCG)
// are the same because they all go through the helpers below.
//
// The order, for n entries on a grid of G workgroups of NT threads:
//   1. thread t of workgroup b accumulates the entries b*NT + t + m*G*NT, m = 0, 1, ..., in that
//      order, into an accumulator that starts at +0.0 (written out at each site: the loop body is
//      the kernel's own work);
//   2. wave_sum: the 64-lane xor butterfly, offsets 32, 16, 8, 4, 2, 1 (every lane gets the total);
//   3. the NT/64 wave totals are added left to right, wave 0 first: one partial per workgroup;
//   4. partials_total: one workgroup sums the G partials, thread t taking the partials t, t + NT,
//      ... in that order (strided_sum), then steps 2 and 3 again.
//
// Step 3 is spelled `t = red[0]; t += red[1]; ...`. The kernels used to spell it either
// ((red[0] + red[1]) + red[2]) + red[3] or `t = 0.0; t += red[i]`, and mirrored each other's
// spelling to stay bitwise. The two differ only if red[0] is -0.0 (0.0 + -0.0 is +0.0), and a sum
// is -0.0 only if both operands are: every accumulator of step 1 starts at +0.0, so no thread's sum,
// no butterfly result and no wave total is ever -0.0, and 0.0 + red[0] is bitwise red[0].
//
// The LDS array of the wave totals is the caller's and is passed in. A helper has exactly one
// barrier, between the posts and the reads; a caller that posts into the same array again while
// other waves may still be reading it puts its own barrier in between.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mlamg {

// Constants shared by kernels that must partition alike to stay bitwise.
// Columns a thread carries in the per-column reductions (spmm.hip, seg_mv.hip, block PCG): the
// tile only groups columns, but the three share tile_sum and its red[NT / 64][kColTile].
constexpr int kColTile = 8;
// Cap of the norm grids (norm2, norm2_mv, norm2_seg_mv): the grid sets which rows a thread walks,
// so a column's or a segment's norm equals the single-vector norm only under the same cap.
constexpr int kNormGridCap = 1024;
// The fixed grid of the sums behind the mean removals (remove_mean, _mv, _seg_mv) and of LSQR's
// vector kernels, whatever n: same reason.
constexpr int kSumGrid = 512;

// Workgroups of `threads` for n entries: one per `threads` entries, at least one, at most cap.
__host__ __device__ inline int reduce_grid(int64_t n, int threads, int cap) {
  const int64_t nb = (n + threads - 1) / threads;
  return (int)(nb < 1 ? 1 : nb > cap ? cap : nb);
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// s = p[start] + p[start+step] + ... in that order (bitwise a plain strided loop), with the loads
// issued 8 at a time: a one-workgroup reduction over tens of thousands of partials is otherwise
// a chain of dependent memory round trips.
__device__ __forceinline__ double strided_sum(const double* __restrict__ p, int n, int start,
                                              int step) {
  double s = 0.0;
  int i = start;
  for (; i + 7 * step < n; i += 8 * step) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[i + u * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; i < n; i += step) s += p[i];
  return s;
}

// step 3 on posted wave totals, after the barrier
template <int NT>
__device__ __forceinline__ double waves_total(const double* red) {
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) t += red[w];
  return t;
}

// steps 2 and 3 of a workgroup of NT threads, red[NT / 64]; every thread gets the total
template <int NT>
__device__ __forceinline__ double block_sum_all(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return waves_total<NT>(red);
}

// the same; thread 0 gets the total (the others 0.0 and read nothing)
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return threadIdx.x == 0 ? waves_total<NT>(red) : 0.0;
}

// steps 2 and 3 for a tile of kColTile accumulators per thread, red[NT / 64][kColTile]: thread
// c < kColTile gets column c's total if it asks for it (`mine`: the column exists and is wanted;
// the others get 0.0 and read nothing)
template <int NT>
__device__ __forceinline__ double tile_sum(const double (&acc)[kColTile], double (*red)[kColTile],
                                           bool mine) {
#pragma unroll
  for (int c = 0; c < kColTile; ++c) {
    const double w = wave_sum(acc[c]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = w;
  }
  __syncthreads();
  double t = 0.0;
  if (mine) {
    t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t += red[w][threadIdx.x];
  }
  return t;
}

// step 4 by a whole workgroup of NT threads over np partials; thread 0 / every thread gets it
template <int NT>
__device__ __forceinline__ double partials_total(const double* __restrict__ p, int np,
                                                 double* red) {
  return block_sum<NT>(strided_sum(p, np, threadIdx.x, NT), red);
}
template <int NT>
__device__ __forceinline__ double partials_total_all(const double* __restrict__ p, int np,
                                                     double* red) {
  return block_sum_all<NT>(strided_sum(p, np, threadIdx.x, NT), red);
}

}  // namespace mlamg
