// GNN inference for learned aggregates and interpolation: the layers of
// ns/model/agg_interp.py FullAggNet.forward (:432-486) — AggNet's TAGConv/InstanceNorm/MLP
// node scorer, MPNN's NNConv/InstanceNorm/edge models (CNet, PNet) — on the device, fp32 like
// the reference (torch_geometric 2.x semantics, restated; torch_geometric is absent here).
//
// A graph is the CSR pattern of A (graph_from_matrix[_basic], ns/model/data.py:22-46): edge e =
// stored entry (i, j) in row-major order, source i = edge_index[0], target j = edge_index[1];
// messages flow source -> target and are summed at the target in edge order (the CSR of the
// transpose lists a target's incoming edges with ascending source), so every aggregation is
// deterministic. Dense layers use torch's Linear layout (weight [out, in], y = x W^T + b).
#include "common.hpp"
#include "reduce.hpp"

#include <rocprim/rocprim.hpp>

namespace mlamg {
namespace {

constexpr int kT = 256;

// Every kernel walks its items with this loop: block b takes items [b * per, (b + 1) * per),
// this thread item `sub` of them, then the block strides on by the whole grid. blocks() below
// sizes (and caps) the grid; the loop covers whatever the cap leaves, so no launch truncates
// its index range. per and gridDim are block-uniform: where `sub` is too (a wave per item, a
// block per tile) the whole wave / block leaves the loop together.
#define MLAMG_GRID_STRIDE(i, n, per, sub)                                  \
  for (int64_t i = (int64_t)blockIdx.x * (per) + (sub); i < (int64_t)(n); \
       i += (int64_t)gridDim.x * (per))

// A population stack (the *_pop entries): `members` equal copies of one base stack end to end,
// member p = blockIdx.y owning rows [p M, (p + 1) M) and edges [p E, (p + 1) E), its tensor of
// every parameter at ptr + p * pstride (0: shared weights). The three weight-consuming kernels
// move their per-item pointers to the member's part and their weights to the member's tensors
// once, then walk the member's items in x exactly as on a stack of their own: a block works for
// one member, no tile straddles two, and an item's arithmetic does not see p. Node and edge ids
// (src, tgt, tptr, teid) are ids of the whole stack, so X and msg stay where they are. The
// single entries are members = 1 (blockIdx.y = 0: every shift is zero).
__device__ __forceinline__ const float* member(const float* w, int64_t pstride) {
  return w ? w + (int64_t)blockIdx.y * pstride : w;
}

// Y[m][n] = beta * Y[m][n] + sum_k X[m][k] W[n][k] (+ b[n]) -> act -> (+ R[m][n or 0]).
// A block stages W^T in LDS (K <= 160, N <= 64) and takes 256 / NP rows at a time, NP = N
// rounded up to a power of two; lane n of a row reads W^T[k][n] (consecutive: no conflicts) and
// the row's X[m][k] (one address: broadcast). M: rows per member.
__global__ void k_linear(const float* __restrict__ X, int64_t M, int K, const float* __restrict__ W,
                         const float* __restrict__ b, int64_t pstride, int N, int NP, int act,
                         float beta, const float* __restrict__ R, int rc, float* __restrict__ Y) {
  extern __shared__ float wt[];  // K x N
  const int64_t row0 = (int64_t)blockIdx.y * M;
  W = member(W, pstride);
  b = member(b, pstride);
  X += row0 * K;
  Y += row0 * N;
  if (R) R += row0 * rc;
  for (int q = threadIdx.x; q < K * N; q += kT) {
    const int k = q / N, n = q % N;
    wt[q] = W[(int64_t)n * K + k];
  }
  __syncthreads();
  const int rows = kT / NP;
  const int r = threadIdx.x / NP, n = threadIdx.x % NP;
  if (n >= N) return;
  MLAMG_GRID_STRIDE(m, M, rows, r) {
    const float* x = X + m * K;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc = fmaf(x[k], wt[k * N + n], acc);
    if (b) acc = acc + b[n];
    float y = beta != 0.0f ? beta * Y[m * N + n] + acc : acc;
    if (act == 1) y = fmaxf(y, 0.0f);
    if (R) y = y + R[m * rc + (rc == 1 ? 0 : n)];
    Y[m * N + n] = y;
  }
}

// y_i = sum over incoming edges e (tptr/teid: edges by target, ascending source) of
// w_e x_src(e); a wave per target, lane f < F
__global__ void k_propagate(const int32_t* __restrict__ tptr, const int32_t* __restrict__ teid,
                            const int32_t* __restrict__ src, const float* __restrict__ w,
                            const float* __restrict__ X, int64_t n, int F, float* __restrict__ Y) {
  const int f = threadIdx.x & 63;
  if (f >= F) return;
  MLAMG_GRID_STRIDE(i, n, kT / 64, threadIdx.x / 64) {
    float acc = 0.0f;
    for (int32_t q = tptr[i]; q < tptr[i + 1]; ++q) {
      const int32_t e = teid[q];
      acc = fmaf(w[e], X[(int64_t)src[e] * F + f], acc);
    }
    Y[i * F + f] = acc;
  }
}

// gcn_norm without self loops (TAGConv normalize=True): deg_j = sum of w over edges with
// target j; w'_e = deg^-1/2[src] w_e deg^-1/2[tgt] (inf -> 0)
__global__ void k_deg_isqrt(const int32_t* __restrict__ tptr, const int32_t* __restrict__ teid,
                            const float* __restrict__ w, int64_t n, float* __restrict__ dis) {
  MLAMG_GRID_STRIDE(j, n, kT, threadIdx.x) {
    float d = 0.0f;
    for (int32_t q = tptr[j]; q < tptr[j + 1]; ++q) d += w[teid[q]];
    const float r = 1.0f / sqrtf(d);
    dis[j] = isinf(r) ? 0.0f : r;
  }
}
__global__ void k_gcn_weight(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                             const float* __restrict__ w, int64_t E, int wstride,
                             const float* __restrict__ dis, float* __restrict__ wn) {
  MLAMG_GRID_STRIDE(e, E, kT, threadIdx.x) wn[e] = (dis[src[e]] * w[e * wstride]) * dis[tgt[e]];
}

// instance norm over the nodes of a segment, per channel (affine False, biased variance, eps):
// item = (segment g, channel f), a block per item; rows seg[g] .. seg[g + 1] of the stack, or the
// one segment [0, n) when seg is null. The sums run in double over the block's strided rows,
// then the wave, then the four wave partials in order: a segment's result depends on its own
// rows alone, wherever it sits in a stack.
__global__ void k_inorm_seg(const float* __restrict__ Xs, const int64_t* __restrict__ seg,
                            int64_t n_rows, int64_t items, int F, float eps,
                            float* __restrict__ Ys) {
  __shared__ double red[kT / 64];
  MLAMG_GRID_STRIDE(it, items, 1, 0) {  // `it` is block-uniform: the block strides together
    // one segment: items = F, so the item is the channel (no 64-bit divide, no offset loads)
    const int64_t g = seg ? it / F : 0;
    const int f = seg ? (int)(it % F) : (int)it;
    const int64_t a = seg ? seg[g] : 0, n = seg ? seg[g + 1] - a : n_rows;
    const float* X = Xs + a * F;
    float* Y = Ys + a * F;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kT) s += X[i * F + f];
    const double mean = block_sum_all<kT>(s, red) / (double)n;
    __syncthreads();
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kT) {
      const double d = X[i * F + f] - mean;
      v += d * d;
    }
    const double vt = block_sum_all<kT>(v, red);
    const float inv = (float)(1.0 / sqrt(vt / (double)n + (double)eps));
    const float mf = (float)mean;
    for (int64_t i = threadIdx.x; i < n; i += kT) Y[i * F + f] = (X[i * F + f] - mf) * inv;
    __syncthreads();  // every wave has read red before the next item overwrites it
  }
}

// NNConv messages, the edge network fused in: per edge e (features ea[e][0..fe)),
//   h1 = relu(L1 ea + c1) (4), h2 = relu(L2 h1 + c2) (16), W_e = relu(L3 h2 + c3) [Fin x Fout],
//   msg[e][o] = sum_i x_src[i] W_e[i][o]   (NNConv.message: x_j @ weight.view(-1, in, out))
// A block: 64 edges (one per lane) x up to 4 output blocks of 16 (one per wave): every lane of a
// wave reads the same L3 row (broadcast), its own source row. E: edges per member.
__global__ void k_nnconv_msg(const int32_t* __restrict__ src, const float* __restrict__ ea,
                             int64_t E, int fe, const float* __restrict__ L1,
                             const float* __restrict__ c1, const float* __restrict__ L2,
                             const float* __restrict__ c2, const float* __restrict__ L3,
                             const float* __restrict__ c3, int64_t pstride,
                             const float* __restrict__ X, int Fin, int Fout,
                             float* __restrict__ msg) {
  const int lane = threadIdx.x & 63, ob = threadIdx.x >> 6;
  const int o0 = ob * 16;
  if (o0 >= Fout) return;
  const int no = min(16, Fout - o0);
  const int64_t edge0 = (int64_t)blockIdx.y * E;
  L1 = member(L1, pstride), c1 = member(c1, pstride);
  L2 = member(L2, pstride), c2 = member(c2, pstride);
  L3 = member(L3, pstride), c3 = member(c3, pstride);
  src += edge0;
  ea += edge0 * fe;
  msg += edge0 * Fout;
  MLAMG_GRID_STRIDE(e0, E, 64, 0) {  // a tile of 64 edges; the block strides together
    const int64_t e = e0 + lane;
    const bool live = e < E;
    const int64_t ee = live ? e : 0;
    float h1[4], h2[16];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float s = 0.0f;
      for (int t = 0; t < fe; ++t) s = fmaf(L1[a * fe + t], ea[ee * fe + t], s);
      h1[a] = fmaxf(s + c1[a], 0.0f);
    }
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) s = fmaf(L2[a * 4 + t], h1[t], s);
      h2[a] = fmaxf(s + c2[a], 0.0f);
    }
    const float* xs = X + (int64_t)src[ee] * Fin;
    float acc[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = 0.0f;
    for (int i = 0; i < Fin; ++i) {
      const float xi = xs[i];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (u < no) {
          const int row = i * Fout + o0 + u;
          const float* l = L3 + (int64_t)row * 16;
          float s = 0.0f;
#pragma unroll
          for (int t = 0; t < 16; ++t) s = fmaf(l[t], h2[t], s);
          const float w = fmaxf(s + c3[row], 0.0f);
          acc[u] = fmaf(xi, w, acc[u]);
        }
      }
    }
    if (live) {
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (u < no) msg[e * Fout + o0 + u] = acc[u];
    }
  }
}

// out[i][o] = act(sum_{incoming e} msg[e][o] + root[i][o] + bias[o]) (+ R[i][o or 0]); n: rows
// per member
__global__ void k_nnconv_aggr(const int32_t* __restrict__ tptr, const int32_t* __restrict__ teid,
                              const float* __restrict__ msg, const float* __restrict__ root,
                              const float* __restrict__ bias, int64_t pstride, int64_t n, int F,
                              int act, const float* __restrict__ R, int rc,
                              float* __restrict__ Y) {
  const int f = threadIdx.x & 63;
  if (f >= F) return;
  const int64_t row0 = (int64_t)blockIdx.y * n;
  bias = member(bias, pstride);
  tptr += row0;
  root += row0 * F;
  Y += row0 * F;
  if (R) R += row0 * rc;
  MLAMG_GRID_STRIDE(i, n, kT / 64, threadIdx.x / 64) {
    float s = 0.0f;
    for (int32_t q = tptr[i]; q < tptr[i + 1]; ++q) s += msg[(int64_t)teid[q] * F + f];
    float y = (s + root[i * F + f]) + bias[f];
    if (act == 1) y = fmaxf(y, 0.0f);
    if (R) y = y + R[i * rc + (rc == 1 ? 0 : f)];
    Y[i * F + f] = y;
  }
}

// smallEdgeModel (agg_interp.py:37-55) and MPNN's post-ops (:124-141): a wave per edge,
//   in = [x_src (F) | x_tgt (F) | ea (fe)], h = relu(W1 in + b1) (H <= 64, lane o),
//   h = LayerNorm(h) * g + beta (eps 1e-5, biased variance), y_c = W2[c] . h + b2[c] (C <= 4),
//   out = act(y) (+ R[e][c or 0]). E: edges per member.
__global__ void k_edge_mlp(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                           const float* __restrict__ X, int F, const float* __restrict__ ea,
                           int fe, int64_t E, const float* __restrict__ W1,
                           const float* __restrict__ b1, int H, const float* __restrict__ g,
                           const float* __restrict__ beta, const float* __restrict__ W2,
                           const float* __restrict__ b2, int64_t pstride, int C, int act,
                           const float* __restrict__ R, int rc, float* __restrict__ out) {
  extern __shared__ float w1t[];  // K x H, K = 2F + fe
  const int K = 2 * F + fe;
  const int64_t edge0 = (int64_t)blockIdx.y * E;
  W1 = member(W1, pstride), b1 = member(b1, pstride);
  g = member(g, pstride), beta = member(beta, pstride);
  W2 = member(W2, pstride), b2 = member(b2, pstride);
  src += edge0;
  tgt += edge0;
  ea += edge0 * fe;
  out += edge0 * C;
  if (R) R += edge0 * rc;
  for (int q = threadIdx.x; q < K * H; q += kT) w1t[q] = W1[(int64_t)(q % H) * K + q / H];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // e is the same in all 64 lanes of a wave, so a wave stays whole through the shuffles and
  // leaves the loop (after the barrier above) as one
  MLAMG_GRID_STRIDE(e, E, kT / 64, threadIdx.x / 64) {
    const float* xs = X + (int64_t)src[e] * F;
    const float* xt = X + (int64_t)tgt[e] * F;
    const float* a = ea + e * fe;
    float h = 0.0f;
    if (lane < H) {
      for (int k = 0; k < F; ++k) h = fmaf(xs[k], w1t[k * H + lane], h);
      for (int k = 0; k < F; ++k) h = fmaf(xt[k], w1t[(F + k) * H + lane], h);
      for (int k = 0; k < fe; ++k) h = fmaf(a[k], w1t[(2 * F + k) * H + lane], h);
      h = fmaxf(h + b1[lane], 0.0f);
    }
    const float mean = wave_sum(lane < H ? h : 0.0f) / (float)H;
    const float d = lane < H ? h - mean : 0.0f;
    const float var = wave_sum(d * d) / (float)H;
    const float hn = lane < H ? (d / sqrtf(var + 1e-5f)) * g[lane] + beta[lane] : 0.0f;
    for (int c = 0; c < C; ++c) {
      float y = wave_sum(lane < H ? hn * W2[c * H + lane] : 0.0f) + b2[c];
      if (act == 1) y = fmaxf(y, 0.0f);
      if (R) y = y + R[e * rc + (rc == 1 ? 0 : c)];
      if (lane == 0) out[e * C + c] = y;
    }
  }
}

// top-k. The key word of a score: ascending words = descending scores under IEEE comparison
// (the two zeros are one score, so between them the node index decides, not the sign bit).
__device__ __forceinline__ uint32_t topk_word(float s) {
  uint32_t u = __float_as_uint(s);
  if ((u << 1) == 0u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending order of the float
  return ~u;
}
// key = segment id | score word (seg null: one segment); the node index rides along as the
// value. The radix sort is stable and the input is in ascending node order, so equal scores of a
// segment stay in ascending index.
__global__ void k_topk_seg_keys(const float* __restrict__ s, const int64_t* __restrict__ seg,
                                int64_t nb, int64_t n, uint64_t* __restrict__ key,
                                int32_t* __restrict__ val) {
  MLAMG_GRID_STRIDE(i, n, kT, threadIdx.x) {
    const uint64_t g = seg ? (uint64_t)seg_of(seg, nb, i) : 0;
    key[i] = (g << 32) | (uint64_t)topk_word(s[i]);
    val[i] = (int32_t)i;
  }
}
// entry t of idx belongs to segment g = seg_of(kptr, t) and is that segment's (t - kptr[g])-th
// best: position seg[g] + t - kptr[g] of the sorted stack (kptr null: one segment from 0, so
// position t). idx is nullable.
__global__ void k_topk_seg_mark(const int32_t* __restrict__ sorted, const int64_t* __restrict__ seg,
                                const int64_t* __restrict__ kptr, int64_t nb, int64_t K,
                                float* __restrict__ vec, int32_t* __restrict__ idx) {
  MLAMG_GRID_STRIDE(t, K, kT, threadIdx.x) {
    int64_t pos = t;
    if (kptr) {
      const int64_t g = seg_of(kptr, nb, t);
      pos = seg[g] + (t - kptr[g]);
    }
    const int32_t i = sorted[pos];
    vec[i] = 1.0f;
    if (idx) idx[t] = i;
  }
}

// The grid of a launch over n items, `per` to a block. The cap keeps the grid within HIP's limit
// on threads per launch; MLAMG_GRID_STRIDE in every kernel covers the items beyond it.
inline unsigned blocks(int64_t n, int per) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 1 << 20));
}
// The same for n items per member with the members in y: they share the cap, so the whole grid
// is no larger than a single launch's (16 blocks per member at 65535 members; the grid-stride
// loop covers the rest). Sharing the cap is a choice for safety, not a tuned one: no other
// split of the grid between x and y has been measured.
inline dim3 blocks(int64_t n, int per, int members) {
  return dim3((unsigned)std::max<int64_t>(
                  1, std::min<int64_t>((n + per - 1) / per, (1 << 20) / members)),
              (unsigned)members);
}

// What a *_pop entry refuses beyond its single entry's own limits: per = rows or edges per
// member (two of them for the NNConv), whose stack-wide ids are int32. The Python layers call
// the *_pop entries for every graph object, a stack of one member included, so these refusals
// (and the *_pop entries' NULL checks, which the single NNConv and edge-model entries do not
// make) also apply to ordinary Graph / GraphBatch inference. GraphBatch itself refuses stacks of
// 2^31 - 1 rows or edges, so no stack it can build is turned away here; the single C entries
// keep their own, wider limits.
int pop_limits(int members, int64_t pstride, int64_t per_a, int64_t per_b) {
  MLAMG_REQUIRE(members >= 1 && members <= 65535, "population: 1 <= members <= 65535");
  MLAMG_REQUIRE(pstride >= 0, "population: pstride >= 0");
  for (int64_t per : {per_a, per_b})
    MLAMG_REQUIRE(per >= 0 && per < INT32_MAX && per * members < INT32_MAX,
                  "population: members * rows and members * edges must stay below 2^31 - 1");
  return MLAMG_OK;
}

// The three weight-consuming layers on `members` members; the single entries are members = 1.
int linear_run(const float* X, int64_t M, int members, int K, const float* W, const float* b,
               int64_t pstride, int N, int act, float beta, const float* R, int rc, float* Y,
               void* stream) {
  MLAMG_REQUIRE(M >= 0 && K >= 1 && K <= 160 && N >= 1 && N <= 64, "linear: K <= 160, N <= 64");
  MLAMG_REQUIRE(W && (M == 0 || (X && Y)) && (!R || rc == 1 || rc == N), "linear: bad arguments");
  if (M == 0) return MLAMG_OK;
  int NP = 1;
  while (NP < N) NP <<= 1;
  const int rows = kT / NP;
  hipLaunchKernelGGL(k_linear, blocks(M, rows, members), dim3(kT), sizeof(float) * K * N,
                     S(stream), X, M, K, W, b, pstride, N, NP, act, beta, R, rc, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int nnconv_run(const int32_t* tptr, const int32_t* teid, const int32_t* src, const float* ea,
               int64_t E, int members, int fe, const float* L1, const float* c1, const float* L2,
               const float* c2, const float* L3, const float* c3, int64_t pstride, const float* X,
               int64_t n, int Fin, int Fout, const float* root, const float* bias, int act,
               const float* R, int rc, float* msg_tmp, float* Y, void* stream) {
  MLAMG_REQUIRE(Fout >= 1 && Fout <= 64 && Fin >= 1 && fe >= 1, "nnconv: Fout <= 64");
  MLAMG_REQUIRE(root && bias && msg_tmp && Y, "NULL argument");
  hipStream_t s = S(stream);
  if (E > 0)
    hipLaunchKernelGGL(k_nnconv_msg, blocks(E, 64, members), dim3(kT), 0, s, src, ea, E, fe, L1,
                       c1, L2, c2, L3, c3, pstride, X, Fin, Fout, msg_tmp);
  hipLaunchKernelGGL(k_nnconv_aggr, blocks(n, kT / 64, members), dim3(kT), 0, s, tptr, teid,
                     msg_tmp, root, bias, pstride, n, Fout, act, R, rc, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int edge_mlp_run(const int32_t* src, const int32_t* tgt, const float* X, int F, const float* ea,
                 int fe, int64_t E, int members, const float* W1, const float* b1, int H,
                 const float* g, const float* beta, const float* W2, const float* b2,
                 int64_t pstride, int C, int act, const float* R, int rc, float* out,
                 void* stream) {
  MLAMG_REQUIRE(H >= 1 && H <= 64 && C >= 1 && C <= 4 && 2 * F + fe <= 160, "edge mlp: sizes");
  if (E == 0) return MLAMG_OK;
  hipLaunchKernelGGL(k_edge_mlp, blocks(E, kT / 64, members), dim3(kT),
                     sizeof(float) * (2 * F + fe) * H, S(stream), src, tgt, X, F, ea, fe, E, W1,
                     b1, H, g, beta, W2, b2, pstride, C, act, R, rc, out);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

// top-k of every segment of a stack of n rows (seg_ptr / k_ptr null: one segment, its k = K):
// one stable sort of (segment id | score word, node index) pairs over the bits in use, then the
// K marks. Everything lives in one cached block: keys in | keys out | values in | values out |
// the sort's own storage. Asynchronous on s.
int topk_run(const float* scores, const int64_t* seg_ptr, const int64_t* k_ptr, int64_t nb,
             int64_t n, int64_t K, float* vec, int32_t* idx, hipStream_t s) {
  int seg_bits = 0;
  while ((int64_t(1) << seg_bits) < nb) ++seg_bits;
  size_t tb = 0;
  MLAMG_HIP(rocprim::radix_sort_pairs(nullptr, tb, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                      (int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0,
                                      32 + seg_bits, s));
  const size_t kb = (sizeof(uint64_t) * (size_t)n + 255) / 256 * 256;
  const size_t vb = (sizeof(int32_t) * (size_t)n + 255) / 256 * 256;
  char* base = static_cast<char*>(scratch(2 * kb + 2 * vb + tb + 256, 19));
  MLAMG_REQUIRE(base, "topk: scratch allocation failed");
  uint64_t* k0 = reinterpret_cast<uint64_t*>(base);
  uint64_t* k1 = reinterpret_cast<uint64_t*>(base + kb);
  int32_t* v0 = reinterpret_cast<int32_t*>(base + 2 * kb);
  int32_t* v1 = reinterpret_cast<int32_t*>(base + 2 * kb + vb);
  void* tmp = base + 2 * kb + 2 * vb;
  hipLaunchKernelGGL(k_topk_seg_keys, dim3(blocks(n, kT)), dim3(kT), 0, s, scores, seg_ptr, nb, n,
                     k0, v0);
  MLAMG_HIP(hipGetLastError());
  MLAMG_HIP(rocprim::radix_sort_pairs(tmp, tb, k0, k1, v0, v1, (size_t)n, 0, 32 + seg_bits, s));
  MLAMG_HIP(hipMemsetAsync(vec, 0, sizeof(float) * n, s));
  if (K > 0)
    hipLaunchKernelGGL(k_topk_seg_mark, dim3(blocks(K, kT)), dim3(kT), 0, s, v1, seg_ptr, k_ptr, nb,
                       K, vec, idx);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

}  // namespace
}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_gnn_linear(const float* X, int64_t M, int K, const float* W, const float* b, int N,
                     int act, float beta, const float* R, int rc, float* Y, void* stream) {
  return linear_run(X, M, 1, K, W, b, 0, N, act, beta, R, rc, Y, stream);
}

int mlamg_gnn_linear_pop(const float* X, int64_t M, int members, int K, const float* W,
                         const float* b, int64_t pstride, int N, int act, float beta,
                         const float* R, int rc, float* Y, void* stream) {
  MLAMG_TRY(pop_limits(members, pstride, M, 0));
  return linear_run(X, M, members, K, W, b, pstride, N, act, beta, R, rc, Y, stream);
}

int mlamg_gnn_gcn_norm(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                       const int32_t* tgt, const float* w, int64_t n, int64_t E, float* dis_tmp,
                       float* wn, void* stream) {
  MLAMG_REQUIRE(n >= 0 && E >= 0 && tptr && dis_tmp, "gcn_norm: NULL argument");
  MLAMG_REQUIRE(E == 0 || (teid && src && tgt && w && wn), "gcn_norm: NULL edge argument");
  hipStream_t s = S(stream);
  hipLaunchKernelGGL(k_deg_isqrt, dim3(blocks(n, kT)), dim3(kT), 0, s, tptr, teid, w, n, dis_tmp);
  if (E > 0)
    hipLaunchKernelGGL(k_gcn_weight, dim3(blocks(E, kT)), dim3(kT), 0, s, src, tgt, w, E, 1,
                       dis_tmp, wn);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_propagate(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                        const float* w, const float* X, int64_t n, int F, float* Y,
                        void* stream) {
  MLAMG_REQUIRE(F >= 1 && F <= 64, "propagate: F <= 64");
  hipLaunchKernelGGL(k_propagate, dim3(blocks(n, kT / 64)), dim3(kT), 0, S(stream), tptr, teid,
                     src, w, X, n, F, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_instance_norm(const float* X, int64_t n, int F, float eps, float* Y, void* stream) {
  MLAMG_REQUIRE(n >= 1 && F >= 1, "instance norm: empty input");
  hipLaunchKernelGGL(k_inorm_seg, dim3(blocks(F, 1)), dim3(kT), 0, S(stream), X,
                     (const int64_t*)nullptr, n, (int64_t)F, F, eps, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_instance_norm_seg(const float* X, const int64_t* seg_ptr,
                                const int64_t* seg_ptr_host, int64_t nb, int F, float eps,
                                float* Y, void* stream) {
  MLAMG_REQUIRE(nb >= 0 && F >= 1, "instance norm (segmented): nb >= 0, F >= 1");
  if (nb == 0) return MLAMG_OK;
  MLAMG_REQUIRE(X && Y && seg_ptr, "instance norm (segmented): NULL argument");
  MLAMG_REQUIRE(nb <= INT64_MAX / F, "instance norm (segmented): nb * F overflows");
  std::vector<int64_t> seg;
  MLAMG_TRY(host_ptr(seg_ptr, seg_ptr_host, nb, 1, S(stream), seg, "instance norm (segmented)"));
  const int64_t items = nb * (int64_t)F;
  // one segment: its bounds are known here, so the kernel does not read the offsets
  hipLaunchKernelGGL(k_inorm_seg, dim3(blocks(items, 1)), dim3(kT), 0, S(stream), X,
                     nb == 1 ? nullptr : seg_ptr, seg[nb], items, F, eps, Y);
  MLAMG_HIP(hipGetLastError());
  return MLAMG_OK;
}

int mlamg_gnn_topk(const float* scores, int64_t n, int64_t k, float* vec, int32_t* idx,
                   void* stream) {
  MLAMG_REQUIRE(scores && vec && k >= 0 && k <= n, "topk: bad arguments");
  MLAMG_REQUIRE(n < INT32_MAX, "topk: too many scores for int32 node ids");
  hipStream_t s = S(stream);
  if (n > 0) MLAMG_TRY(topk_run(scores, nullptr, nullptr, 1, n, k, vec, idx, s));
  MLAMG_HIP(hipStreamSynchronize(s));
  return MLAMG_OK;
}

int mlamg_gnn_topk_seg(const float* scores, const int64_t* seg_ptr, const int64_t* seg_ptr_host,
                       const int64_t* k_ptr, const int64_t* k_ptr_host, int64_t nb, float* vec,
                       int32_t* idx, void* stream) {
  MLAMG_REQUIRE(nb >= 0, "topk (segmented): negative segment count");
  if (nb == 0) return MLAMG_OK;
  MLAMG_REQUIRE(seg_ptr && k_ptr, "topk (segmented): NULL argument");
  hipStream_t s = S(stream);
  std::vector<int64_t> seg, kp;
  MLAMG_TRY(host_ptr(seg_ptr, seg_ptr_host, nb, 0, s, seg, "topk (segmented) seg_ptr"));
  MLAMG_TRY(host_ptr(k_ptr, k_ptr_host, nb, 0, s, kp, "topk (segmented) k_ptr"));
  for (int64_t g = 0; g < nb; ++g)
    MLAMG_REQUIRE(kp[g + 1] - kp[g] <= seg[g + 1] - seg[g],
                  "topk (segmented): a segment asks for more than its own rows (k_g <= n_g)");
  const int64_t n = seg[nb], K = kp[nb];
  MLAMG_REQUIRE(n < INT32_MAX, "topk (segmented): stack too large for int32 node ids");
  if (n == 0) return MLAMG_OK;
  MLAMG_REQUIRE(scores && vec && (K == 0 || idx), "topk (segmented): NULL argument");
  if (nb == 1) return topk_run(scores, nullptr, nullptr, 1, n, K, vec, idx, s);  // as above
  return topk_run(scores, seg_ptr, k_ptr, nb, n, K, vec, idx, s);
}

int mlamg_gnn_nnconv(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                     const float* ea, int64_t E, int fe, const float* L1, const float* c1,
                     const float* L2, const float* c2, const float* L3, const float* c3,
                     const float* X, int64_t n, int Fin, int Fout, const float* root,
                     const float* bias, int act, const float* R, int rc, float* msg_tmp,
                     float* Y, void* stream) {
  return nnconv_run(tptr, teid, src, ea, E, 1, fe, L1, c1, L2, c2, L3, c3, 0, X, n, Fin, Fout,
                    root, bias, act, R, rc, msg_tmp, Y, stream);
}

int mlamg_gnn_nnconv_pop(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                         const float* ea, int64_t E, int members, int fe, const float* L1,
                         const float* c1, const float* L2, const float* c2, const float* L3,
                         const float* c3, int64_t pstride, const float* X, int64_t n, int Fin,
                         int Fout, const float* root, const float* bias, int act, const float* R,
                         int rc, float* msg_tmp, float* Y, void* stream) {
  MLAMG_TRY(pop_limits(members, pstride, n, E));
  MLAMG_REQUIRE(tptr && X && (E == 0 || (teid && src && ea && L1 && c1 && L2 && c2 && L3 && c3)),
                "nnconv: NULL argument");
  return nnconv_run(tptr, teid, src, ea, E, members, fe, L1, c1, L2, c2, L3, c3, pstride, X, n,
                    Fin, Fout, root, bias, act, R, rc, msg_tmp, Y, stream);
}

int mlamg_gnn_edge_mlp(const int32_t* src, const int32_t* tgt, const float* X, int F,
                       const float* ea, int fe, int64_t E, const float* W1, const float* b1,
                       int H, const float* g, const float* beta, const float* W2,
                       const float* b2, int C, int act, const float* R, int rc, float* out,
                       void* stream) {
  return edge_mlp_run(src, tgt, X, F, ea, fe, E, 1, W1, b1, H, g, beta, W2, b2, 0, C, act, R, rc,
                      out, stream);
}

int mlamg_gnn_edge_mlp_pop(const int32_t* src, const int32_t* tgt, const float* X, int F,
                           const float* ea, int fe, int64_t E, int members, const float* W1,
                           const float* b1, int H, const float* g, const float* beta,
                           const float* W2, const float* b2, int64_t pstride, int C, int act,
                           const float* R, int rc, float* out, void* stream) {
  MLAMG_TRY(pop_limits(members, pstride, E, 0));
  MLAMG_REQUIRE(E == 0 || (src && tgt && X && ea && W1 && b1 && g && beta && W2 && b2 && out),
                "edge mlp: NULL argument");
  return edge_mlp_run(src, tgt, X, F, ea, fe, E, members, W1, b1, H, g, beta, W2, b2, pstride, C,
                      act, R, rc, out, stream);
}

}  // extern "C"
