// Block GMRES: gmres.hip's restarted, left-preconditioned MGS GMRES on every column of a
// row-major n x k block of right-hand sides at once (mlamg_gmres_mv). Column j of
// X, its step count, info and history are bitwise what mlamg_gmres returns on column j alone.
//
// The columns run in lock-step: every column shares the inner step `col`, so one SpMM
// (spmm_set_mv), one zero-guess block cycle (hier_coarse_cycle_mv) and one launch per
// Gram-Schmidt dot / update serve all k columns. What keeps the bits:
//  - the dots walk the rows as k_gm_part does (nb = reduce_grid(n, 256, 1024) workgroups on
//    blockIdx.x, thread t of workgroup b takes the rows b*256 + t + m*nb*256; reduce.hpp's order
//    from there) with one accumulator per column of a tile of kColTile columns (blockIdx.y),
//    partials at [col * nb + b]; the consumer sums a column's partials in gm_total's order
//    (col_total: one wave plays the four waves of gm_total's workgroup). No arrival counters;
//  - the updates are k_gm_axmy_p's, k_gm_scale_dev's and k_gm_update's expressions per column;
//  - the Hessenberg work of a step is gm_arnoldi_step (gmres.hpp), one workgroup per column, on
//    the column's own Hessenberg columns, Givens pairs, rotated right-hand side, status block,
//    ptol, ||b|| and history; the restart boundary's triangular solve (gm_small_solve) and the
//    outer test with the gh-8400 ptol adaptation run on the host per column.
// A column whose inner stop fires is frozen for the rest of that restart cycle (done[c]: its w, V
// and state are no longer written); the workgroup that stops the last running column raises the
// all-columns flag, the one status the host reads per step. A column that has converged, has
// ||b|| = 0, starts below atol or broke down is frozen for good: it enters later cycles with
// done[c] = 1 and a zero length in the update, so its x is no longer written. The operator and
// the preconditioner still stream frozen columns (their results are not read); the Krylov blocks
// are zeroed at the start of a solve so that such a column never carries a stale NaN into the
// preconditioner's coarse solve.
#include "gmres.hpp"
#include "hier.hpp"

namespace mlamg {

// int32 state of a restart cycle: [0] every column's inner stop has fired, [1] columns stopped,
// done[c] at [kGmFlags + c]
constexpr int kGmFlags = 8;

// bit c set: column c0 + c of the tile exists and runs (done == nullptr: every column runs); read
// by one thread for the whole workgroup, ends with a barrier
__device__ __forceinline__ unsigned gmmv_live(const int32_t* done, int c0, int k) {
  __shared__ unsigned s_live;
  if (threadIdx.x == 0) {
    unsigned live = 0;
    for (int c = 0; c < kColTile && c0 + c < k; ++c)
      if (!done || !done[c0 + c]) live |= 1u << c;
    s_live = live;
  }
  __syncthreads();
  return s_live;
}

// gm_total(partial, nb) computed by one wave: lane l carries the sums of gm_total's threads
// l, l + 64, l + 128, l + 192 (the same strided order), each goes through the same butterfly, and
// the four wave sums are added in red[]'s order. All lanes get the total.
__device__ __forceinline__ double col_total(const double* __restrict__ partial, int nb, int lane) {
  double w[kGmThreads / 64];
#pragma unroll
  for (int u = 0; u < kGmThreads / 64; ++u)
    w[u] = wave_sum(strided_sum(partial, nb, lane + 64 * u, kGmThreads));
  return waves_total<kGmThreads>(w);
}

// k_gm_part per column: partials of u.v -> partial[col * nb + b] (running columns)
__global__ __launch_bounds__(kGmThreads) void k_gmmv_dot(const double* __restrict__ U, int64_t ldu,
                                                        const double* __restrict__ V, int64_t ldv,
                                                        int64_t n, int k,
                                                        double* __restrict__ partial,
                                                        const int32_t* done) {
  __shared__ double red[kGmThreads / 64][kColTile];
  const int c0 = blockIdx.y * kColTile;
  const unsigned live = gmmv_live(done, c0, k);
  if (!live) return;
  double acc[kColTile];
#pragma unroll
  for (int c = 0; c < kColTile; ++c) acc[c] = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kGmThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kGmThreads) {
    const double* u = U + i * ldu + c0;
    const double* v = V + i * ldv + c0;
#pragma unroll
    for (int c = 0; c < kColTile; ++c)
      if ((live >> c) & 1u) acc[c] += u[c] * v[c];
  }
  const bool mine = threadIdx.x < kColTile && ((live >> threadIdx.x) & 1u);
  const double t = tile_sum<kGmThreads>(acc, red, mine);
  if (mine) partial[(int64_t)(c0 + threadIdx.x) * gridDim.x + blockIdx.x] = t;
}

// out[c] = the total of column c's partials (a wave each): the norms the host reads
__global__ __launch_bounds__(64) void k_gmmv_total(const double* __restrict__ partial, int nb,
                                                   double* __restrict__ out) {
  const int c = blockIdx.x;
  const double t = col_total(partial + (int64_t)c * nb, nb, threadIdx.x);
  if (threadIdx.x == 0) out[c] = t;
}

// k_gm_axmy_p per column: w -= c v with c = the dot k_gmmv_dot left in partial (every workgroup
// sums it; workgroup 0 of the tile also stores it, the Hessenberg entry coef[col * ldc])
__global__ __launch_bounds__(kGmThreads) void k_gmmv_axmy(double* __restrict__ W,
                                                         const double* __restrict__ V, int64_t n,
                                                         int k, const double* __restrict__ partial,
                                                         double* __restrict__ coef, int ldc,
                                                         const int32_t* done) {
  __shared__ double tot[kColTile];
  const int c0 = blockIdx.y * kColTile;
  const unsigned live = gmmv_live(done, c0, k);
  if (!live) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < kColTile / (kGmThreads / 64); ++u) {
    const int c = wv + (kGmThreads / 64) * u;
    if ((live >> c) & 1u) {
      const double t = col_total(partial + (int64_t)(c0 + c) * gridDim.x, gridDim.x, lane);
      if (lane == 0) tot[c] = t;
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < kColTile && ((live >> threadIdx.x) & 1u))
    coef[(int64_t)(c0 + threadIdx.x) * ldc] = tot[threadIdx.x];
  double cf[kColTile];
#pragma unroll
  for (int c = 0; c < kColTile; ++c) cf[c] = ((live >> c) & 1u) ? tot[c] : 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kGmThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kGmThreads) {
    double* w = W + i * (int64_t)k + c0;
    const double* v = V + i * (int64_t)k + c0;
#pragma unroll
    for (int c = 0; c < kColTile; ++c)
      if ((live >> c) & 1u) w[c] = w[c] - cf[c] * v[c];
  }
}

// k_gm_arnoldi per column (workgroup c): the column's stop marks it done, and the workgroup that
// stops the last running column raises the all-columns flag
__global__ __launch_bounds__(kGmThreads) void k_gmmv_arnoldi(
    int col, int restart, int k, const double* __restrict__ scal, const double* __restrict__ p_h0,
    const double* __restrict__ p_h1, int np, double* __restrict__ Hd, double* __restrict__ giv,
    double* __restrict__ S, double* __restrict__ st, double eps, const double* __restrict__ ptol,
    const double* __restrict__ bnrm2, double* __restrict__ hist, int hist_cap, int32_t* fl) {
  __shared__ double red[kGmThreads / 64];
  const int c = blockIdx.x;
  if (fl[kGmFlags + c]) return;
  const double w0 = gm_total(p_h0 + (int64_t)c * np, np, red);
  __syncthreads();
  const double w1 = gm_total(p_h1 + (int64_t)c * np, np, red);
  if (threadIdx.x != 0) return;
  const int ldh = restart + 1;
  if (gm_arnoldi_step(col, ldh, scal + (int64_t)c * (restart + 2), w0, w1,
                      Hd + (int64_t)c * restart * ldh, giv + (int64_t)c * 2 * restart,
                      S + (int64_t)c * ldh, st + 8 * c, eps, ptol[c], bnrm2[c],
                      hist ? hist + (int64_t)c * hist_cap : nullptr, hist_cap)) {
    fl[kGmFlags + c] = 1;
    if (atomicAdd(fl + 1, 1) == k - 1) fl[0] = 1;
  }
}

// k_gm_scale / k_gm_scale_dev per column: y = x * (1 / d) with d = d[col * ldd]
__global__ __launch_bounds__(kGmThreads) void k_gmmv_scale(double* __restrict__ Y,
                                                          const double* __restrict__ X, int64_t n,
                                                          int k, const double* __restrict__ d,
                                                          int ldd, const int32_t* done) {
  const int c0 = blockIdx.y * kColTile;
  const unsigned live = gmmv_live(done, c0, k);
  if (!live) return;
  double inv[kColTile];
#pragma unroll
  for (int c = 0; c < kColTile; ++c)
    inv[c] = ((live >> c) & 1u) ? 1.0 / d[(int64_t)(c0 + c) * ldd] : 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kGmThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kGmThreads) {
    double* y = Y + i * (int64_t)k + c0;
    const double* x = X + i * (int64_t)k + c0;
#pragma unroll
    for (int c = 0; c < kColTile; ++c)
      if ((live >> c) & 1u) y[c] = x[c] * inv[c];
  }
}

// k_gm_update per column: x_c += sum_{j < m[c]} y_c[j] v_j (j ascending); m[c] = 0: x_c is not
// written. Krylov block j lies at V + j * vstride.
__global__ __launch_bounds__(kGmThreads) void k_gmmv_update(double* __restrict__ X, int64_t ldx,
                                                           const double* __restrict__ V,
                                                           int64_t vstride, int64_t n, int k,
                                                           const double* __restrict__ y, int ldy,
                                                           const int32_t* __restrict__ m) {
  const int c0 = blockIdx.y * kColTile;
  int mc[kColTile], mmax = 0;
#pragma unroll
  for (int c = 0; c < kColTile; ++c) {
    mc[c] = c0 + c < k ? m[c0 + c] : 0;
    mmax = max(mmax, mc[c]);
  }
  if (mmax == 0) return;
  for (int64_t i = blockIdx.x * (int64_t)kGmThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kGmThreads) {
    double t[kColTile];
#pragma unroll
    for (int c = 0; c < kColTile; ++c) t[c] = 0.0;
    for (int j = 0; j < mmax; ++j) {
      const double* v = V + j * vstride + i * (int64_t)k + c0;
#pragma unroll
      for (int c = 0; c < kColTile; ++c)
        if (j < mc[c]) t[c] += y[(int64_t)(c0 + c) * ldy + j] * v[c];
    }
    double* x = X + i * ldx + c0;
#pragma unroll
    for (int c = 0; c < kColTile; ++c)
      if (mc[c] > 0) x[c] = x[c] + t[c];
  }
}

// x_c = b_c (a zero right-hand side: scipy returns b)
__global__ __launch_bounds__(kGmThreads) void k_gmmv_copycol(double* __restrict__ X, int64_t ldx,
                                                            const double* __restrict__ B,
                                                            int64_t ldb, int64_t n, int c) {
  for (int64_t i = blockIdx.x * (int64_t)kGmThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kGmThreads)
    X[i * ldx + c] = B[i * ldb + c];
}

namespace {
struct GmMvWork {
  double* V = nullptr;  // restart + 1 Krylov blocks, vstride apart
  int64_t vstride = 0;
  double* AV = nullptr;
  double* R = nullptr;
  double* partial = nullptr;  // k x nb partials of the current MGS dot, [col * nb + b]
  double* p_h0 = nullptr;     // ... of ||w||^2 before / after the projections
  double* p_h1 = nullptr;
  double* scal = nullptr;  // per column restart + 2: the MGS coefficients
  double* y = nullptr;     // per column restart + 1: solution of the small triangular system
  // one region, mirrored on the host: the first four are sent at the start of a restart cycle,
  // S, st and Hd are read back at its end
  double* ptol = nullptr;  // k
  double* d = nullptr;     // k: ||v_0|| before its normalisation
  double* S = nullptr;     // per column restart + 1
  double* st = nullptr;    // per column 8 (gm_arnoldi_step)
  double* Hd = nullptr;    // per column restart x (restart + 1)
  double* giv = nullptr;   // per column 2 restart
  double* bnrm2 = nullptr;  // k
  double* nrm = nullptr;    // k: squared norms for the host
  double* hist = nullptr;   // per column hist_cap
  int32_t* fl = nullptr;    // kGmFlags + k (see kGmFlags)
  int32_t* m = nullptr;     // k: Krylov vectors in each column's update
};

size_t gmmv_layout(GmMvWork* W, char* base, int64_t n, int k, int restart, int nb, int hist_cap) {
  Carver c{base};
  const int64_t ldh = restart + 1;
  W->vstride = (int64_t)(((sizeof(double) * (size_t)std::max<int64_t>(n, 1) * k) + 255) &
                         ~size_t(255)) / (int64_t)sizeof(double);
  W->V = c.take(W->vstride * (restart + 1));
  W->AV = c.take(W->vstride);
  W->R = c.take(W->vstride);
  W->partial = c.take((int64_t)k * nb);
  W->p_h0 = c.take((int64_t)k * nb);
  W->p_h1 = c.take((int64_t)k * nb);
  W->scal = c.take((int64_t)k * (restart + 2));
  W->y = c.take((int64_t)k * ldh);
  W->ptol = c.take((int64_t)k * (2 + ldh + 8 + restart * ldh + 2 * restart));
  W->d = W->ptol + k;
  W->S = W->d + k;
  W->st = W->S + (int64_t)k * ldh;
  W->Hd = W->st + 8 * (int64_t)k;
  W->giv = W->Hd + (int64_t)k * restart * ldh;
  W->bnrm2 = c.take(k);
  W->nrm = c.take(k);
  W->hist = c.take((int64_t)k * std::max(hist_cap, 1));
  W->fl = reinterpret_cast<int32_t*>(c.take((kGmFlags + 2 * k + 1) / 2));
  W->m = W->fl + kGmFlags + k;
  return c.off;
}

struct GmCol {  // a column's outer state (gmres_impl's locals)
  bool live = true;
  double bnrm2 = 0.0, atol = 0.0, ptol = 0.0, ptol_max_factor = 1.0, presid = 0.0, rnorm = 0.0;
  bool breakdown = false;
  int iters = 0;
};
}  // namespace

static int gmres_mv_impl(const mlamg_csr* A, mlamg_hier* M, const double* B, int64_t ldb,
                         double* X, int64_t ldx, int k, double rtol, int restart, int maxiter,
                         bool x_zero, int32_t* info, int32_t* iters_out, double* presid_hist,
                         int hist_cap, hipStream_t s) {
  const int64_t n = A->n_rows;
  if (restart <= 0) restart = 20;
  restart = (int)std::min<int64_t>(restart, std::max<int64_t>(n, 1));
  if (maxiter <= 0) maxiter = (int)std::min<int64_t>(INT32_MAX, 10 * std::max<int64_t>(n, 1));
  const int ldh = restart + 1;
  const int nb = reduce_grid(n, kGmThreads, kGmMaxBlocks);
  const bool canon = A->vec_width != 0;  // a VECTOR-format A is summed in the canonical order
  GmMvWork W;
  const size_t total = gmmv_layout(&W, nullptr, n, k, restart, nb, hist_cap);
  void* mem = nullptr;
  MLAMG_TRY(hier_workspace(M, total, &mem));
  gmmv_layout(&W, static_cast<char*>(mem), n, k, restart, nb, hist_cap);
  MLAMG_TRY(hier_prepare_ext(M));
  MLAMG_HIP(hipMemsetAsync(W.V, 0, sizeof(double) * (size_t)W.vstride * (restart + 1), s));
  const dim3 grid(nb, (k + kColTile - 1) / kColTile), thr(kGmThreads);
  auto Vk = [&](int j) { return W.V + (int64_t)j * W.vstride; };
  const size_t row = sizeof(double) * (size_t)k;

  auto dot = [&](const double* U, int64_t ldu, const double* V, int64_t ldv, double* partial,
                 const int32_t* done) {
    hipLaunchKernelGGL(k_gmmv_dot, grid, thr, 0, s, U, ldu, V, ldv, n, k, partial, done);
  };
  std::vector<double> nrm(k);
  auto norms = [&](const double* U, int64_t ldu) -> int {  // nrm[c] = sqrt(u_c . u_c)
    dot(U, ldu, U, ldu, W.partial, nullptr);
    hipLaunchKernelGGL(k_gmmv_total, dim3(k), dim3(64), 0, s, W.partial, nb, W.nrm);
    MLAMG_HIP(hipGetLastError());
    MLAMG_HIP(hipMemcpyAsync(nrm.data(), W.nrm, row, hipMemcpyDeviceToHost, s));
    MLAMG_HIP(hipStreamSynchronize(s));
    for (double& v : nrm) v = std::sqrt(v);
    return MLAMG_OK;
  };
  double* Z = nullptr;  // the preconditioner's result, in M's block workspace
  auto psolve = [&](const double* in) -> int {  // one block V-cycle from X = 0
    return hier_coarse_cycle_mv(M, in, &Z, k, s, nullptr, true);
  };
  auto resid = [&]() -> int {  // R = B - A X
    return residual_mv(A, B, ldb, X, ldx, W.R, k, k, s, nullptr, canon);
  };

  std::vector<GmCol> C(k);
  MLAMG_TRY(norms(B, ldb));
  int live = 0;
  for (int c = 0; c < k; ++c) {
    C[c].bnrm2 = nrm[c];
    C[c].atol = rtol * nrm[c];  // _get_atol_rtol: max(atol = 0, rtol * ||b||)
    if (nrm[c] == 0.0) {        // scipy returns postprocess(b)
      C[c].live = false;
      hipLaunchKernelGGL(k_gmmv_copycol, dim3(nb), thr, 0, s, X, ldx, B, ldb, n, c);
      MLAMG_HIP(hipGetLastError());
    }
    live += C[c].live;
  }
  const double eps = 2.220446049250313e-16;
  bool have_z = false;  // Z == M R
  if (live) {
    for (int c = 0; c < k; ++c) nrm[c] = C[c].bnrm2;
    MLAMG_HIP(hipMemcpyAsync(W.bnrm2, nrm.data(), row, hipMemcpyHostToDevice, s));
    MLAMG_HIP(hipMemcpy2DAsync(W.R, row, B, sizeof(double) * ldb, row, n,
                               hipMemcpyDeviceToDevice, s));
    MLAMG_TRY(psolve(W.R));
    MLAMG_TRY(norms(Z, k));  // ||M b||
    for (int c = 0; c < k; ++c)
      C[c].ptol = nrm[c] * std::min(C[c].ptol_max_factor, C[c].atol / C[c].bnrm2);
    if (x_zero) {
      have_z = true;  // r_0 = b, already in R
    } else {
      MLAMG_TRY(resid());
    }
    MLAMG_TRY(norms(W.R, k));
    for (int c = 0; c < k; ++c) {
      if (C[c].live && nrm[c] < C[c].atol) {
        C[c].rnorm = nrm[c];
        C[c].live = false;
        --live;
      }
    }
  }
  const size_t n_up = (size_t)k * (2 + ldh + 8), n_back = (size_t)k * (ldh + 8 + restart * ldh);
  std::vector<double> hu((size_t)k * (2 + ldh + 8 + restart * ldh), 0.0), y((size_t)k * ldh, 0.0);
  std::vector<int32_t> fl(kGmFlags + k, 0), m(k, 0);
  double* hS = hu.data() + 2 * (size_t)k;
  double* hst = hS + (size_t)k * ldh;
  double* hH = hst + 8 * (size_t)k;
  int32_t* done = W.fl + kGmFlags;
  for (int iteration = 0; iteration < maxiter && live; ++iteration) {
    if (!have_z) MLAMG_TRY(psolve(W.R));
    have_z = false;
    MLAMG_TRY(norms(Z, k));
    // the cycle's small state: per column ptol, ||v_0||, the rotated right-hand side and the
    // step count; a column that is frozen for good starts the cycle done
    std::fill(hu.begin(), hu.begin() + n_up, 0.0);
    std::fill(fl.begin(), fl.end(), 0);
    for (int c = 0; c < k; ++c) {
      hu[c] = C[c].ptol;
      hu[k + c] = C[c].live ? nrm[c] : 1.0;
      hS[(size_t)c * ldh] = nrm[c];
      hst[8 * c + 4] = (double)C[c].iters;
      fl[kGmFlags + c] = C[c].live ? 0 : 1;
    }
    fl[1] = k - live;
    MLAMG_HIP(hipMemcpyAsync(W.ptol, hu.data(), sizeof(double) * n_up, hipMemcpyHostToDevice, s));
    MLAMG_HIP(hipMemcpyAsync(W.fl, fl.data(), sizeof(int32_t) * fl.size(), hipMemcpyHostToDevice,
                             s));
    hipLaunchKernelGGL(k_gmmv_scale, grid, thr, 0, s, Vk(0), Z, n, k, W.d, 1, done);
    MLAMG_HIP(hipGetLastError());
    for (int col = 0; col < restart; ++col) {
      MLAMG_TRY(spmm_set_mv(A, Vk(col), k, W.AV, k, k, 1.0, 0.0, s, nullptr, canon));
      MLAMG_TRY(psolve(W.AV));  // w = M A v, orthogonalised in place
      dot(Z, k, Z, k, W.p_h0, done);  // h0^2
      for (int j = 0; j <= col; ++j) {  // modified Gram-Schmidt, coefficients on the device
        dot(Vk(j), k, Z, k, W.partial, done);
        hipLaunchKernelGGL(k_gmmv_axmy, grid, thr, 0, s, Z, Vk(j), n, k, W.partial, W.scal + j,
                           restart + 2, done);
      }
      dot(Z, k, Z, k, W.p_h1, done);
      hipLaunchKernelGGL(k_gmmv_arnoldi, dim3(k), thr, 0, s, col, restart, k, W.scal, W.p_h0,
                         W.p_h1, nb, W.Hd, W.giv, W.S, W.st, eps, W.ptol, W.bnrm2,
                         presid_hist ? W.hist : nullptr, hist_cap, W.fl);
      hipLaunchKernelGGL(k_gmmv_scale, grid, thr, 0, s, Vk(col + 1), Z, n, k, W.st + 1, 8, done);
      MLAMG_HIP(hipGetLastError());
      int32_t all = 0;
      MLAMG_HIP(hipMemcpyAsync(&all, W.fl, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      MLAMG_HIP(hipStreamSynchronize(s));
      if (all) break;
    }
    MLAMG_HIP(hipMemcpyAsync(hS, W.S, sizeof(double) * n_back, hipMemcpyDeviceToHost, s));
    MLAMG_HIP(hipStreamSynchronize(s));
    // restart boundary: each column's triangular solve from its own last column index
    for (int c = 0; c < k; ++c) {
      m[c] = 0;
      if (!C[c].live) continue;
      const double* stc = hst + 8 * c;
      C[c].presid = stc[0];
      C[c].breakdown = stc[2] != 0.0;
      C[c].iters = (int)stc[4];
      const int last = (int)stc[3];
      gm_small_solve(hH + (size_t)c * restart * ldh, ldh, hS + (size_t)c * ldh, last,
                     y.data() + (size_t)c * ldh);
      m[c] = last + 1;
    }
    MLAMG_HIP(hipMemcpyAsync(W.y, y.data(), sizeof(double) * y.size(), hipMemcpyHostToDevice, s));
    MLAMG_HIP(hipMemcpyAsync(W.m, m.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gmmv_update, grid, thr, 0, s, X, ldx, W.V, W.vstride, n, k, W.y, ldh,
                       W.m);
    MLAMG_HIP(hipGetLastError());
    MLAMG_TRY(resid());
    MLAMG_TRY(norms(W.R, k));
    for (int c = 0; c < k; ++c) {
      GmCol& G = C[c];
      if (!G.live) continue;
      G.rnorm = nrm[c];
      if (G.rnorm <= G.atol || G.breakdown) {
        G.live = false;
        --live;
        continue;
      }
      if (G.presid <= G.ptol)
        G.ptol_max_factor = std::max(eps, 0.25 * G.ptol_max_factor);
      else
        G.ptol_max_factor = std::min(1.0, 1.5 * G.ptol_max_factor);
      G.ptol = G.presid * std::min(G.ptol_max_factor, G.atol / G.rnorm);
    }
  }
  std::vector<double> hist;
  if (presid_hist) {
    hist.resize((size_t)k * hist_cap);
    MLAMG_HIP(hipMemcpyAsync(hist.data(), W.hist, sizeof(double) * hist.size(),
                             hipMemcpyDeviceToHost, s));
  }
  MLAMG_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < k; ++c) {
    info[c] = C[c].bnrm2 == 0.0 || C[c].rnorm <= C[c].atol ? 0 : maxiter;
    iters_out[c] = C[c].iters;
    for (int j = 0; presid_hist && j < std::min(C[c].iters, hist_cap); ++j)
      presid_hist[(size_t)j * k + c] = hist[(size_t)c * hist_cap + j];
  }
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_gmres_mv(const mlamg_csr* A, mlamg_hier* M, const double* B, int64_t ldb, double* X,
                   int64_t ldx, int k, double rtol, int restart, int maxiter, int x_is_zero,
                   int32_t* info, int32_t* inner_iters, double* presid_hist_host, int hist_cap,
                   void* stream) {
  MLAMG_REQUIRE(A, "A is NULL");
  MLAMG_REQUIRE(M, "M is NULL");
  MLAMG_REQUIRE(B, "B is NULL");
  MLAMG_REQUIRE(X, "X is NULL");
  MLAMG_REQUIRE(info, "info is NULL");
  MLAMG_REQUIRE(inner_iters, "inner_iters is NULL");
  MLAMG_MV_K(k);
  MLAMG_REQUIRE(ldb >= k, "ldb < k");
  MLAMG_REQUIRE(ldx >= k, "ldx < k");
  MLAMG_REQUIRE(B != X, "B and X must differ");
  MLAMG_REQUIRE(rtol >= 0.0, "rtol >= 0 required");
  MLAMG_REQUIRE(!presid_hist_host || hist_cap >= 0, "hist_cap < 0");
  MLAMG_REQUIRE(A->n_rows == A->n_cols, "square matrix required");
  MLAMG_REQUIRE(hier_fine_rows(M) == A->n_rows, "preconditioner hierarchy does not match A");
  if (A->n_rows == 0) {
    for (int c = 0; c < k; ++c) info[c] = inner_iters[c] = 0;
    return MLAMG_OK;
  }
  if (!presid_hist_host || hist_cap == 0) {
    presid_hist_host = nullptr;
    hist_cap = 0;
  }
  return gmres_mv_impl(A, M, B, ldb, X, ldx, k, rtol, restart, maxiter, x_is_zero != 0, info,
                       inner_iters, presid_hist_host, hist_cap, S(stream));
}

}  // extern "C"
