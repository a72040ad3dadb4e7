// The wide GNN layers of ns/model/ali_interp.py InterpolationNetwork: a
// ResidualBlock of 20 TAGConv(K=5) layers up to 256 channels and an EdgeModel 513 -> 256 -> ... ->
// 1 with a LayerNorm after every block. gnn.hip's kernels stop at 64 channels (a wave lane per
// channel, W^T whole in LDS); the kernels here take rows of up to 256 channels, and the dense
// products go through the f32-input matrix cores. fp32 like the reference; graph conventions as
// in gnn.hip (edges in row-major order, tptr/teid = each target's incoming edges).
#include "common.hpp"
#include "reduce.hpp"

namespace mlamg {
namespace {

constexpr int kT = 256;
constexpr int kWideF = 256;          // widest row of the wave-per-row kernels
constexpr int kFPL = kWideF / 64;    // features a lane carries: f = lane + 64 c

// gnn.hip's item loop: block b takes items [b * per, (b + 1) * per), this thread item `sub` of
// them, then the block strides on by the whole grid (per and gridDim are block-uniform).
#define MLAMG_GRID_STRIDE(i, n, per, sub)                                  \
  for (int64_t i = (int64_t)blockIdx.x * (per) + (sub); i < (int64_t)(n); \
       i += (int64_t)gridDim.x * (per))

inline unsigned blocks(int64_t n, int per) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 1 << 20));
}

// ------------------------------------------------------------------------------ linear (MFMA)
// Y = beta * Y + X W^T (+ b) -> act -> (+ R), k_linear's epilogue. A block of 4 waves (2 x 2)
// owns a (64 Q) x (64 Q) tile of Y, a wave Q x Q quadrants of 32 x 32, each in 16 accumulator
// registers of v_mfma_f32_32x32x2_f32; X and W arrive in LDS 32 k at a time (rows padded to 33
// floats: the 32 rows a half-wave reads land in 32 banks). Lane l feeds A[i = l & 31][k = l >> 5]
// and B[k = l >> 5][j = l & 31]; the instruction computes fma(a_k1, b_k1, fma(a_k0, b_k0, C))
// with one rounding per product, so an output is the fmaf chain over k = 0 .. K-1 from +0.0 that
// k_linear computes, whatever Q. Rows, columns and k beyond M, N and K are zeros in LDS: a padded
// product adds +0.0 (it can only turn a -0.0 sum into +0.0), and no load leaves the arrays.
// Q = 1: with Q = 2 (128 x 128 tiles, a quarter of the LDS reads and global loads per product) the
// kernel needs 210 VGPRs, one wave per SIMD is left to hide its loads, and it measured 23-27
// TFLOP/s against 33-43 at (M, 256, 256), M = 65,536 and 262,144.
using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kBK = 32, kLd = kBK + 1;
constexpr int kQ = 1;

__global__ __launch_bounds__(kT) void k_linear_mfma(
    const float* __restrict__ X, int64_t M, int K, const float* __restrict__ W,
    const float* __restrict__ b, int N, int act, float beta, const float* __restrict__ R, int rc,
    float* __restrict__ Y, int64_t tiles, int ntn) {
  constexpr int Q = kQ, kB = 64 * Q;  // tile rows and columns
  __shared__ float xs[kB * kLd];
  __shared__ float ws[kB * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32 * Q, wn = (wave & 1) * 32 * Q;
  const int li = lane & 31, lk = lane >> 5;
  MLAMG_GRID_STRIDE(t, tiles, 1, 0) {  // t is block-uniform: the block strides together
    const int64_t m0 = (t / ntn) * kB;
    const int n0 = (int)(t % ntn) * kB;
    f32x16 acc[Q][Q];
#pragma unroll
    for (int i = 0; i < Q; ++i)
#pragma unroll
      for (int j = 0; j < Q; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kBK) {
#pragma unroll
      for (int u = 0; u < kB * kBK / kT; ++u) {
        const int q = threadIdx.x + u * kT;
        const int r = q >> 5, kk = q & 31;
        const int k = k0 + kk;
        const int64_t m = m0 + r;
        const int n = n0 + r;
        xs[r * kLd + kk] = (m < M && k < K) ? X[m * K + k] : 0.0f;
        ws[r * kLd + kk] = (n < N && k < K) ? W[(int64_t)n * K + k] : 0.0f;
      }
      __syncthreads();
      const int kend = min(kBK, K - k0);  // an odd kend reads the zero at kend (<= 31)
      const float* xa = xs + (wm + li) * kLd + lk;
      const float* wb = ws + (wn + li) * kLd + lk;
      for (int kk = 0; kk < kend; kk += 2) {
        float a[Q], bq[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) a[i] = xa[i * 32 * kLd + kk];
#pragma unroll
        for (int j = 0; j < Q; ++j) bq[j] = wb[j * 32 * kLd + kk];
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
          for (int j = 0; j < Q; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bq[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < Q; ++i)
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const int n = n0 + wn + j * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (m < M && n < N) {
            float v = acc[i][j][r];
            if (b) v = v + b[n];
            float y = beta != 0.0f ? beta * Y[m * N + n] + v : v;
            if (act == 1) y = fmaxf(y, 0.0f);
            if (R) y = y + R[m * rc + (rc == 1 ? 0 : n)];
            Y[m * N + n] = y;
          }
        }
      }
  }
}

// ----------------------------------------------------------------------------------- propagate
// k_propagate with up to kFPL features per lane: a wave per target, the same edge-order fmaf
// chain per feature
__global__ void k_propagate_wide(const int32_t* __restrict__ tptr, const int32_t* __restrict__ teid,
                                 const int32_t* __restrict__ src, const float* __restrict__ w,
                                 const float* __restrict__ X, int64_t n, int F,
                                 float* __restrict__ Y) {
  const int lane = threadIdx.x & 63;
  MLAMG_GRID_STRIDE(i, n, kT / 64, threadIdx.x / 64) {
    float acc[kFPL];
#pragma unroll
    for (int c = 0; c < kFPL; ++c) acc[c] = 0.0f;
    for (int32_t q = tptr[i]; q < tptr[i + 1]; ++q) {
      const int32_t e = teid[q];
      const float we = w[e];
      const float* xs = X + (int64_t)src[e] * F;
#pragma unroll
      for (int c = 0; c < kFPL; ++c) {
        const int f = lane + 64 * c;
        if (f < F) acc[c] = fmaf(we, xs[f], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < kFPL; ++c) {
      const int f = lane + 64 * c;
      if (f < F) Y[i * F + f] = acc[c];
    }
  }
}

// ---------------------------------------------------------------------------------- LayerNorm
// LayerNorm of the row a wave holds (h[c] = feature lane + 64 c), in place: mean and biased
// variance in double (the lane's features in order from +0.0, then wave_sum), the normalised
// value rounded once to fp32, then * g + beta in fp32 (null: 1 and 0). Every lane of the wave
// calls it.
__device__ __forceinline__ void layer_norm_row(float (&h)[kFPL], int F, int lane,
                                               const float* __restrict__ g,
                                               const float* __restrict__ beta, float eps) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < kFPL; ++c)
    if (lane + 64 * c < F) s += h[c];
  const double mean = wave_sum(s) / (double)F;
  double v = 0.0;
#pragma unroll
  for (int c = 0; c < kFPL; ++c)
    if (lane + 64 * c < F) {
      const double d = (double)h[c] - mean;
      v += d * d;
    }
  const double inv = 1.0 / sqrt(wave_sum(v) / (double)F + (double)eps);
#pragma unroll
  for (int c = 0; c < kFPL; ++c) {
    const int f = lane + 64 * c;
    if (f < F) {
      const float y = (float)(((double)h[c] - mean) * inv);
      h[c] = y * (g ? g[f] : 1.0f) + (beta ? beta[f] : 0.0f);
    }
  }
}

__global__ void k_layer_norm(const float* __restrict__ X, int64_t rows, int F,
                             const float* __restrict__ g, const float* __restrict__ beta,
                             float eps, const float* __restrict__ R, int act,
                             float* __restrict__ Y) {
  const int lane = threadIdx.x & 63;
  // a row is the same in all lanes of a wave: the wave stays whole through the shuffles
  MLAMG_GRID_STRIDE(i, rows, kT / 64, threadIdx.x / 64) {
    float h[kFPL];
#pragma unroll
    for (int c = 0; c < kFPL; ++c) {
      const int f = lane + 64 * c;
      h[c] = f < F ? X[i * F + f] : 0.0f;
    }
    layer_norm_row(h, F, lane, g, beta, eps);
#pragma unroll
    for (int c = 0; c < kFPL; ++c) {
      const int f = lane + 64 * c;
      if (f < F) {
        float y = h[c];
        if (R) y = y + R[i * F + f];
        if (act == 1) y = fmaxf(y, 0.0f);
        Y[i * F + f] = y;
      }
    }
  }
}

// first EdgeModel block from the node products: a wave per edge
__global__ void k_edge_in(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                          const float* __restrict__ U, const float* __restrict__ V,
                          const float* __restrict__ ea, int64_t E, int H,
                          const float* __restrict__ w, const float* __restrict__ b,
                          const float* __restrict__ g, const float* __restrict__ beta, float eps,
                          float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  MLAMG_GRID_STRIDE(e, E, kT / 64, threadIdx.x / 64) {
    const float* u = U + (int64_t)src[e] * H;
    const float* v = V + (int64_t)tgt[e] * H;
    const float a = ea[e];
    float h[kFPL];
#pragma unroll
    for (int c = 0; c < kFPL; ++c) {
      const int f = lane + 64 * c;
      h[c] = f < H ? ((u[f] + v[f]) + a * w[f]) + b[f] : 0.0f;
    }
    layer_norm_row(h, H, lane, g, beta, eps);
#pragma unroll
    for (int c = 0; c < kFPL; ++c) {
      const int f = lane + 64 * c;
      if (f < H) out[e * H + f] = fmaxf(h[c], 0.0f);
    }
  }
}

// ------------------------------------------------------------------------ |(v - mean) / std|
// reduce.hpp's order on a grid of G = reduce_grid(E, kT, kSumGrid) workgroups: partial sums of
// v, then of (v - mean)^2 with the mean every workgroup totals from the first partials, then
// the map with both totals.
__global__ void k_std_sum(const float* __restrict__ v, int64_t E, double* __restrict__ part) {
  __shared__ double red[kT / 64];
  double s = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < E; e += (int64_t)gridDim.x * kT)
    s += v[e];
  const double t = block_sum<kT>(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ void k_std_var(const float* __restrict__ v, int64_t E, const double* __restrict__ psum,
                          double* __restrict__ part) {
  __shared__ double red[kT / 64];
  const double mean = partials_total_all<kT>(psum, gridDim.x, red) / (double)E;
  __syncthreads();  // every wave has read red before it is posted into again
  double s = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < E; e += (int64_t)gridDim.x * kT) {
    const double d = (double)v[e] - mean;
    s += d * d;
  }
  const double t = block_sum<kT>(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ void k_std_apply(const float* __restrict__ v, int64_t E, const double* __restrict__ psum,
                            const double* __restrict__ pvar, int np, float* __restrict__ out) {
  __shared__ double red[kT / 64];
  const double mean = partials_total_all<kT>(psum, np, red) / (double)E;
  __syncthreads();
  const double inv = 1.0 / sqrt(partials_total_all<kT>(pvar, np, red) / (double)(E - 1));
  MLAMG_GRID_STRIDE(e, E, kT, threadIdx.x) out[e] = (float)fabs(((double)v[e] - mean) * inv);
}

}  // namespace
}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_gnn_linear_wide(const float* X, int64_t M, int K, const float* W, const float* b, int N,
                          int act, float beta, const float* R, int rc, float* Y, void* stream) {
  MLAMG_REQUIRE(M >= 0 && K >= 1 && K <= 1024 && N >= 1 && N <= 256,
                "linear (wide): K <= 1024, N <= 256");
  MLAMG_REQUIRE(beta == 0.0f || beta == 1.0f, "linear (wide): beta must be 0 or 1");
  MLAMG_REQUIRE(W && (M == 0 || (X && Y)) && (!R || rc == 1 || rc == N),
                "linear (wide): bad arguments");
  if (M == 0) return MLAMG_OK;
  const int ntn = (N + 64 * kQ - 1) / (64 * kQ);
  const int64_t tiles = ((M + 64 * kQ - 1) / (64 * kQ)) * ntn;
  hipLaunchKernelGGL(k_linear_mfma, dim3(blocks(tiles, 1)), dim3(kT), 0, S(stream), X, M, K, W, b,
                     N, act, beta, R, rc, Y, tiles, ntn);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_propagate_wide(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                             const float* w, const float* X, int64_t n, int F, float* Y,
                             void* stream) {
  MLAMG_REQUIRE(F >= 1 && F <= kWideF && n >= 0, "propagate (wide): F <= 256");
  if (n == 0) return MLAMG_OK;
  MLAMG_REQUIRE(tptr && X && Y, "propagate (wide): NULL argument");
  hipLaunchKernelGGL(k_propagate_wide, dim3(blocks(n, kT / 64)), dim3(kT), 0, S(stream), tptr,
                     teid, src, w, X, n, F, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_layer_norm(const float* X, int64_t rows, int F, const float* weight,
                         const float* bias, float eps, const float* R, int act, float* Y,
                         void* stream) {
  MLAMG_REQUIRE(F >= 1 && F <= kWideF && rows >= 0, "layer norm: F <= 256");
  if (rows == 0) return MLAMG_OK;
  MLAMG_REQUIRE(X && Y, "layer norm: NULL argument");
  hipLaunchKernelGGL(k_layer_norm, dim3(blocks(rows, kT / 64)), dim3(kT), 0, S(stream), X, rows, F,
                     weight, bias, eps, R, act, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_edge_in(const int32_t* src, const int32_t* tgt, const float* U, const float* V,
                      const float* ea, int64_t E, int H, const float* w, const float* b,
                      const float* g, const float* beta, float eps, float* out, void* stream) {
  MLAMG_REQUIRE(H >= 1 && H <= kWideF && E >= 0, "edge in: H <= 256");
  if (E == 0) return MLAMG_OK;
  MLAMG_REQUIRE(src && tgt && U && V && ea && w && b && out, "edge in: NULL argument");
  hipLaunchKernelGGL(k_edge_in, dim3(blocks(E, kT / 64)), dim3(kT), 0, S(stream), src, tgt, U, V,
                     ea, E, H, w, b, g, beta, eps, out);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_standardize_abs(const float* v, int64_t E, float* out, void* stream) {
  MLAMG_REQUIRE(E >= 2, "standardize: the unbiased std needs E >= 2");
  MLAMG_REQUIRE(v && out, "standardize: NULL argument");
  const int G = reduce_grid(E, kT, kSumGrid);
  double* part = static_cast<double*>(scratch(sizeof(double) * 2 * kSumGrid, 20));
  MLAMG_REQUIRE(part, "standardize: scratch allocation failed");
  hipStream_t s = S(stream);
  hipLaunchKernelGGL(k_std_sum, dim3(G), dim3(kT), 0, s, v, E, part);
  hipLaunchKernelGGL(k_std_var, dim3(G), dim3(kT), 0, s, v, E, part, part + kSumGrid);
  hipLaunchKernelGGL(k_std_apply, dim3(blocks(E, kT)), dim3(kT), 0, s, v, E, part,
                     part + kSumGrid, G, out);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

}  // extern "C"
