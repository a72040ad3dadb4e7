/*
 * mlamg.h — C-ABI of libmlamg_hip.so, the MI355X (gfx950) implementation of ml-amg's AMG V-cycle
 * solve path (nicknytko/ml-amg: ns/lib/multigrid.py, ns/lib/graph.py, ns/lib/sparse.py,
 * ns/preconditioner/MLAMG.py).
 *
 * The reference is pure Python; its "FFI" is the set of Python calls into scipy sparsetools,
 * SuperLU, ARPACK and pyamg amg_core that the hot path makes. Each entry point below names the
 * reference call (file:line) it replaces. The Python side (ml-amg_amd/mlamg/_lib.py) binds these
 * with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch types. int32 CSR indices, fp64 values.
 *  - every vector argument is a DEVICE pointer (e.g. torch.Tensor.data_ptr()) unless named *_host.
 *  - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default.
 *    Calls are asynchronous on it; calls that return a host-visible value synchronise it.
 *  - return 0 on success, a negative MLAMG_E* code on failure; message via mlamg_last_error()
 *    (thread-local). Numerical breakdown (NaN) is not an error: it flows through the results,
 *    as in the reference (utils/common.py:78-81 maps NaN conv factors itself).
 *  - handles own their device memory unless created with MLAMG_WRAP_DEVICE.
 */
#ifndef MLAMG_H_
#define MLAMG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLAMG_OK 0
#define MLAMG_EINVAL -1
#define MLAMG_EHIP -2
#define MLAMG_ENCCL -3
#define MLAMG_ENOMEM -4
#define MLAMG_EUNSUPPORTED -5

/* where the arrays passed to mlamg_csr_create live */
#define MLAMG_COPY_HOST 0    /* host arrays, copied to the device               */
#define MLAMG_COPY_DEVICE 1  /* device arrays, copied                            */
#define MLAMG_WRAP_DEVICE 2  /* device arrays, wrapped (caller keeps them alive) */

typedef struct mlamg_csr mlamg_csr;
typedef struct mlamg_dense mlamg_dense;
typedef struct mlamg_blockdense mlamg_blockdense;
typedef struct mlamg_hier mlamg_hier;
typedef struct mlamg_gs mlamg_gs;
typedef struct mlamg_poly mlamg_poly;
typedef struct mlamg_pcg mlamg_pcg;
typedef struct mlamg_comm mlamg_comm;

/* ---------------------------------------------------------------- runtime */
int mlamg_version(void);
const char* mlamg_last_error(void);
int mlamg_set_device(int dev);
int mlamg_get_device(int* dev);
int mlamg_stream_sync(void* stream);
/* Dispatch-packet kernel timing (no reference counterpart: bench.py's roofline measurement).
 * Arm a timer on the calling thread; the next SpMV-family kernel launch (mlamg_spmv,
 * mlamg_residual, the smoother sweeps and their fused epilogues) records the timer's events in
 * its own dispatch packet and disarms it; elapsed_ms then waits for it and returns that kernel's
 * execution time, as a profiler's kernel trace reports it. A launch recorded into a stream
 * capture never takes the timer. disarm drops an armed timer no launch took (call it after the
 * timed entry point returns: a later, unrelated launch must not take it). */
typedef struct mlamg_timer mlamg_timer;
int mlamg_timer_create(mlamg_timer** out);
int mlamg_timer_destroy(mlamg_timer* t);
int mlamg_timer_arm(mlamg_timer* t);
int mlamg_timer_disarm(void);
int mlamg_timer_elapsed_ms(mlamg_timer* t, float* ms);

/* ---------------------------------------------------------------- CSR handles
 * Replaces the scipy.sparse.csr_matrix objects the reference passes around
 * (ns/lib/multigrid.py:111 A,P; ns/preconditioner/MLAMG.py:103 self.A) and the torch COO
 * conversions of ns/lib/sparse.py:20-32,105-106. */
int mlamg_csr_create(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* indptr,
                     const int32_t* indices, const double* data, int where, mlamg_csr** out);
int mlamg_csr_destroy(mlamg_csr* A);
int mlamg_csr_shape(const mlamg_csr* A, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
int mlamg_csr_device_arrays(const mlamg_csr* A, int32_t** indptr, int32_t** indices,
                            double** data);
/* copy the arrays back to host buffers (indptr n_rows+1, indices/data nnz); syncs */
/* copies of the CSR arrays into caller DEVICE buffers (any may be NULL), async on `stream` */
int mlamg_csr_copy_device(const mlamg_csr* A, int32_t* indptr, int32_t* indices, double* data,
                          void* stream);
int mlamg_csr_download(const mlamg_csr* A, int32_t* indptr_host, int32_t* indices_host,
                       double* data_host);
/* 64-bit fingerprint of the operator's rows, columns and value bits (order-independent sum of
 * per-entry hashes; keys the format autotune's cache, no reference counterpart); syncs */
int mlamg_csr_fingerprint(const mlamg_csr* A, uint64_t* fp_host, void* stream);

/* SpMV storage/kernel of a handle (the CSR arrays always stay; formats add a device copy; a
 * conversion that is refused or fails leaves the handle in the format it had):
 *   CSR_STREAM  LDS-staged row blocks, lane-per-row sums in stored order (scipy's bits)
 *   SELL        SELL-64 slices, lane-per-row sums in stored order (scipy's bits); vec_width > 1
 *               is read as sigma: rows sorted by length inside windows of sigma rows
 *               (SELL-C-sigma; get_format reports sigma in vec_width)
 *   VECTOR      vec_width lanes per row (0 = auto from the mean row length; 64, 128, 256 or
 *               512; <= 2^20 rows), lane-parallel sums in ONE canonical order whatever the width
 *               (512 virtual lanes: lane v sums entries v, v+512, ...; xor butterfly per 64-lane
 *               virtual wave; the 8 wave sums left to right — oracle vec_matvec), for long-row
 *               coarse operators with no scipy counterpart; norm partials per row
 *   AUTO_EXACT  SELL when its padding costs <= 15% extra entries, else CSR_STREAM
 *   SORTED      CSR_STREAM row blocks (<= 512 rows, <= 4096 nonzeros) whose entries are stored
 *               in ascending column order with their CSR slot, so the x gathers of a
 *               wave-instruction hit few cache lines; sums in stored order (scipy's bits).
 *               EUNSUPPORTED if a row has > 4096 nonzeros or a block's columns do not fit
 *               two windows of 2^20 columns */
#define MLAMG_FMT_CSR_STREAM 0
#define MLAMG_FMT_SELL 1
#define MLAMG_FMT_VECTOR 2
#define MLAMG_FMT_AUTO_EXACT 3
#define MLAMG_FMT_SORTED 4
/* SELL_DICT   SELL-64[-sigma] whose elements are 2-byte codes into per-matrix dictionaries of
 *             <= 255 distinct column offsets (col - row) and <= 256 distinct values (bit
 *             patterns): lossless, same products in the same order as SELL (scipy's bits).
 *             For constant-coefficient stencils (C4: 7 offsets, 2 values) the matrix stream is
 *             2 B/nonzero instead of 12. vec_width = sigma as for SELL. EUNSUPPORTED (format
 *             unchanged) when the dictionaries overflow. */
#define MLAMG_FMT_SELL_DICT 5
/* ROWPAT      every row is one of <= 255 distinct patterns (its (col - row, value) sequence in
 *             stored order; C4's 7-point Laplacian: 27 interior/face/edge/corner patterns) held
 *             in LDS tables (<= 2048 padded entries), one byte per row PAIR in HBM: lossless, each row summed
 *             in stored order (scipy's bits). get_format reports the pattern count in
 *             vec_width. EUNSUPPORTED (format unchanged) when the patterns do not fit. */
#define MLAMG_FMT_ROWPAT 6
/* LONG        scipy's order for long rows (coarse Galerkin operators, R = P^T): tiles of
 *             <= 64 consecutive rows / <= 4096 nonzeros over the CSR arrays themselves, one
 *             workgroup each; every row summed left to right by one lane from LDS products with
 *             pipelined reads (csrc/spmv.hip k_csr_long). Bitwise csr_matvec. */
#define MLAMG_FMT_LONG 7
int mlamg_csr_set_format(mlamg_csr* A, int fmt, int vec_width, void* stream);
int mlamg_csr_get_format(const mlamg_csr* A, int* fmt, int* vec_width, int64_t* stored_entries);
/* Attach the level's Jacobi weights dinv_w (device, n_rows) to a ROWPAT operator: checked on the
 * device to be constant over each row-pair pattern (true for the diagonal of a constant-
 * coefficient stencil), after which every epilogue of A whose dinv pointer IS dinv_w takes the
 * values from the pattern table instead of reading the vector (same bits). The caller keeps
 * dinv_w alive and unchanged while attached; NULL detaches; any set_format detaches.
 * EUNSUPPORTED (nothing attached) if A is not ROWPAT or dinv_w is not pattern-constant.
 * Replaces no reference call: an optimisation of the weighted-Jacobi sweep (MLAMG.py:143-146). */
int mlamg_csr_attach_dinv(mlamg_csr* A, const double* dinv_w, void* stream);
/* algorithmic HBM bytes of one y = A@x with the active format: matrix stream as stored (CSR:
 * 12*nnz + 4*(n+1); SELL: 12 B per padded element + slice pointers; SELL_DICT: 2 B per code +
 * tables; SORTED: CSR + block tables; ROWPAT: 1 B per row + tables) + 8*n_cols (x once) + 8*n_rows (y once) */
int mlamg_csr_format_bytes(const mlamg_csr* A, double* bytes);

/* ---------------------------------------------------------------- hot-path sparse ops
 * Each sums a row left-to-right in stored order with separate multiply and add roundings,
 * i.e. exactly scipy sparsetools csr_matvec, so results are bitwise identical to the CPU path. */

/* y = alpha*A@x + beta*y.  A@x: ns/lib/multigrid.py:181,191; MLAMG.py:145,191,194.
 * alpha==1 && beta==0 gives A@x bit for bit. */
int mlamg_spmv(const mlamg_csr* A, const double* x, double* y, double alpha, double beta,
               void* stream);

/* r = b - A@x; if norm2 != NULL, *norm2 (DEVICE scalar) = ||r||_2 (deterministic order).
 * ns/lib/multigrid.py:181,191 (b - A@x), :191 la.norm; MLAMG.py:191,194. */
int mlamg_residual(const mlamg_csr* A, const double* b, const double* x, double* r,
                   double* norm2, void* stream);

/* nu weighted-Jacobi sweeps, MLAMG form: x += Dinv@(b - A@x), Dinv = diag(1/a_ii)*omega
 * pre-scaled (ns/preconditioner/MLAMG.py:104,143-146). x_tmp: scratch of n. Result lands in x. */
int mlamg_jacobi(const mlamg_csr* A, const double* dinv_w, const double* b, double* x,
                 double* x_tmp, int nu, void* stream);

/* nu sweeps of ns/lib/multigrid.py:15-45 form: x += (w*Dinv)@b - ((w*Dinv)@A)@x.
 * M must be the explicit (w*Dinv)@A built by mlamg_csr_scale_rows(reverse=1). */
int mlamg_jacobi_explicit(const mlamg_csr* M, const double* dinv_w, const double* b, double* x,
                          double* x_tmp, int nu, void* stream);

/* r_c = R@r with R = P^T held explicitly (mlamg_transpose). Bitwise equal to scipy's
 * csc_matvec of P.T@r (ns/lib/multigrid.py:181; MLAMG.py:191). */
int mlamg_restrict(const mlamg_csr* R, const double* r, double* r_c, void* stream);

/* x += P@e_c (ns/lib/multigrid.py:181 `x += P @ ...`; MLAMG.py:191). */
int mlamg_prolong_add(const mlamg_csr* P, const double* e_c, double* x, void* stream);

/* dinv_w[i] = (1.0/a_ii)*omega (MLAMG.py:104; multigrid.py:41,104). Missing diagonal -> 1/0. */
int mlamg_diag_inv(const mlamg_csr* A, double omega, double* dinv_w, void* stream);

/* *out (DEVICE scalar) = ||x||_2 (multigrid.py:193 la.norm(x, 2)). */
int mlamg_norm2(const double* x, int64_t n, double* out, void* stream);

/* ---------------------------------------------------------------- setup kernels */
/* R = A^T, columns sorted (used for P.T; multigrid.py:165,181). */
int mlamg_transpose(const mlamg_csr* A, mlamg_csr** out, void* stream);

/* C = A@B with scipy csr_matmat semantics (multigrid.py:107 `smoother @ Agg`):
 * C_ij = 0 + A_ik1*B_k1j + ... over k in the stored order of A's row i, exact zeros dropped, and
 * each output row's columns in csr_matmat's order (reverse order of first appearance), so a
 * later C@x sums in the same order as scipy. */
int mlamg_spgemm(const mlamg_csr* A, const mlamg_csr* B, mlamg_csr** out, void* stream);

/* setup scratch: SpGEMM temporaries are cached device blocks reused across calls; this frees
 * the cached (unused) blocks. freed_bytes nullable. */
int mlamg_scratch_trim(size_t* freed_bytes);
/* device allocation cache (csrc/runtime.cpp): every library buffer comes from size-class lists
 * of released blocks (a hipFree unmaps pages, ~1 ms per buffer). trim really frees the cached
 * blocks; stats reports the cached bytes and the hit / miss counts. Pointers nullable. */
int mlamg_device_cache_trim(size_t* freed_bytes);
int mlamg_device_cache_stats(size_t* cached_bytes, int64_t* hits, int64_t* misses);
/* accumulated wall times (ms) of the Galerkin/SpGEMM phases since the last reset, in the order
 * count, alloc, expand, sort, runsum, emit, finalize, free (n <= 8 entries written) */
int mlamg_setup_phase_times(double* ms_out, int n, int reset);
/* A_c = (R@A)@P, left-associative like `P.T@A@P` (multigrid.py:165; MLAMG.py:121), with R = P^T
 * from mlamg_transpose. Every entry is summed over k ascending, as scipy's CSC kernels do for
 * this expression, so values are bitwise scipy's; output columns sorted ascending. */
int mlamg_galerkin(const mlamg_csr* R, const mlamg_csr* A, const mlamg_csr* P, mlamg_csr** out,
                   void* stream);

/* S = I - (omega*Dinv)@A with scipy rounding/zero-dropping (multigrid.py:104-106). */
int mlamg_sa_smoother(const mlamg_csr* A, double omega, mlamg_csr** out, void* stream);

/* M = diag(d)@A (row scaling). reverse=1: zeros dropped, each row's columns in descending
 * order — the order scipy's csr_matmat emits for dia@csr (multigrid.py:44). reverse=0: A's
 * pattern and stored order kept, nothing dropped — sparsetools csr_scale_rows (pyamg
 * scale_rows, the D^-1 A of evolution_strength_of_connection). */
int mlamg_csr_scale_rows(const mlamg_csr* A, const double* d, int reverse, mlamg_csr** out,
                         void* stream);

/* lambda_max of Dinv@A (ARPACK eigs k=1 'LM' in multigrid.py:105) by Lanczos on the similar
 * symmetric D^-1/2 A D^-1/2 (A symmetric with positive diagonal). *lam_host written; syncs.
 * At most max_iter steps, which may be more than n (no reorthogonalisation: in finite precision
 * the tridiagonal can need more than n rows); scratch for 2 max_iter doubles is allocated. The
 * stop test |theta - theta_prev| <= tol |theta| between checks 32 steps apart is a stagnation
 * test, not an error bound. A row without a stored diagonal entry, or with a zero, negative or
 * non-finite one, gives MLAMG_EINVAL and leaves *lam_host and *iters_host untouched. */
int mlamg_lambda_max_dinvA(const mlamg_csr* A, int max_iter, double tol, uint64_t seed,
                           double* lam_host, int* iters_host, void* stream);

/* strength-of-connection graph (utils/common.py:26,28,29): mode 0 abs, 1 invabs, 2 unit. */
int mlamg_strength(const mlamg_csr* A, int mode, mlamg_csr** out, void* stream);

/* Evolution strength of connection: pyamg.strength.evolution_strength_of_connection(A) at the
 * reference's arguments (B = ones, k = 2, proj_type 'l2', symmetrized; epsilon = the drop
 * tolerance, pyamg default 4.0), as used by utils/common.py:27,30 (csrc/strength.hip). A: CSR with
 * ascending column indices and no explicit zeros; rho = spectral radius of D^-1 A (pyamg
 * estimates it by Arnoldi; the caller supplies it). mode 0: the evolution measure itself,
 * 1: + 0.1 * unit(A) (the reference's 'evolution'), 2: + 1/|A| (the reference's 'olson').
 * *out: new CSR, ascending columns. Syncs. */
int mlamg_evolution_strength(const mlamg_csr* A, double rho, double epsilon, int mode,
                             mlamg_csr** out, void* stream);

/* GNN inference layers of ns/model/agg_interp.py FullAggNet.forward (:432-486), fp32, device
 * pointers (csrc/gnn.hip). Graph = the CSR pattern of A (ns/model/data.py:22-46): edge e = stored
 * entry (src i, tgt j); messages flow src -> tgt; tptr[n+1]/teid[E] list each target's incoming
 * edges, ascending source. Dense weights in torch Linear layout [out, in]; act 0 none, 1 relu; R
 * (nullable) is added after the activation, rc = its columns (1: broadcast). Every launch covers
 * its whole index range whatever n, M or E (int32 edge ids: E < 2^31). A size outside the limit
 * stated at a prototype returns MLAMG_EINVAL and writes nothing. */
/* Y[M][N] = act(beta * Y + X[M][K] W[N][K]^T (+ b[N])) (+ R); beta == 0: Y is not read.
 * Limits: 1 <= K <= 160, 1 <= N <= 64, M >= 0, rc in {1, N} when R is given. */
int mlamg_gnn_linear(const float* X, int64_t M, int K, const float* W, const float* b, int N,
                     int act, float beta, const float* R, int rc, float* Y, void* stream);
/* gcn_norm without self loops (TAGConv normalize=True): deg_j = sum of w over edges with target
 * j, dis_tmp[n] = deg^-1/2 (0 where deg == 0), wn_e = dis[src] w_e dis[tgt]. No size limit. */
int mlamg_gnn_gcn_norm(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                       const int32_t* tgt, const float* w, int64_t n, int64_t E, float* dis_tmp,
                       float* wn, void* stream);
/* Y[i] = sum over incoming edges of w_e X[src_e] (TAGConv propagate, aggr 'add'; a node without
 * incoming edges gets 0). Limits: 1 <= F <= 64. */
int mlamg_gnn_propagate(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                        const float* w, const float* X, int64_t n, int F, float* Y, void* stream);
/* torch_geometric InstanceNorm (affine False, no running stats): per channel over the nodes,
 * (x - mean) / sqrt(biased variance + eps). The kernel of mlamg_gnn_instance_norm_seg on the one
 * segment [0, n). Limits: n >= 1, F >= 1 (no upper limit). */
int mlamg_gnn_instance_norm(const float* X, int64_t n, int F, float eps, float* Y, void* stream);
/* NNConv(Fin, Fout, nn = Linear(fe,4)-ReLU-Linear(4,16)-ReLU-Linear(16,Fin*Fout)-ReLU), aggr
 * 'add', root weight `root` = X W_root^T (precomputed), bias; msg_tmp[E*Fout] scratch (not
 * touched when E == 0). Limits: 1 <= Fout <= 64, Fin >= 1, fe >= 1. */
int mlamg_gnn_nnconv(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                     const float* ea, int64_t E, int fe, const float* L1, const float* c1,
                     const float* L2, const float* c2, const float* L3, const float* c3,
                     const float* X, int64_t n, int Fin, int Fout, const float* root,
                     const float* bias, int act, const float* R, int rc, float* msg_tmp,
                     float* Y, void* stream);
/* smallEdgeModel: Linear(2F+fe, H)-ReLU-LayerNorm(H, eps 1e-5)-Linear(H, C) on
 * [x_src | x_tgt | ea]; E == 0 returns without a launch.
 * Limits: 1 <= H <= 64, 1 <= C <= 4, 2F + fe <= 160. */
int mlamg_gnn_edge_mlp(const int32_t* src, const int32_t* tgt, const float* X, int F,
                       const float* ea, int fe, int64_t E, const float* W1, const float* b1,
                       int H, const float* g, const float* beta, const float* W2,
                       const float* b2, int C, int act, const float* R, int rc, float* out,
                       void* stream);
/* topk_vec (agg_interp.py:14-22): vec[n] = 1 at the k largest scores (ties, -0.0 == +0.0 among
 * them: smaller index first), idx[k] (nullable) = those nodes in that order; the order of NaN
 * scores is unspecified. mlamg_gnn_topk_seg's sort and kernels on one segment, out of the same
 * cached per-thread block: no allocation after the first call of a size.
 * Limits: 0 <= k <= n < 2^31 - 1 (int32 node ids). Syncs. */
int mlamg_gnn_topk(const float* scores, int64_t n, int64_t k, float* vec, int32_t* idx,
                   void* stream);

/* A stack of nb graphs (FullAggNet.forward_batch): rows seg_ptr[g] .. seg_ptr[g + 1] are graph
 * g's nodes. Every *_ptr array is int64[nb + 1] on the DEVICE and starts at 0; its *_host twin
 * is the same array on the host, used to validate the call without reading the device back
 * (NULL: the entry copies the device array back, one synchronisation). The two must be equal.
 *
 * InstanceNorm per graph and channel: segment g of Y is bitwise mlamg_gnn_instance_norm on rows
 * seg_ptr[g] .. seg_ptr[g + 1] of X alone (one kernel serves both: strided double sums, wave
 * sums, the wave partials in order, one workgroup per (graph, channel)). Does not synchronise
 * with the host mirror given. Limits: every segment has >= 1 row, F >= 1 (EINVAL before any
 * launch). */
int mlamg_gnn_instance_norm_seg(const float* X, const int64_t* seg_ptr,
                                const int64_t* seg_ptr_host, int64_t nb, int F, float eps,
                                float* Y, void* stream);
/* topk_vec per graph: vec[n] = 1 at the k_g = k_ptr[g + 1] - k_ptr[g] largest scores of segment
 * g, 0 elsewhere; idx[k_ptr[g] .. k_ptr[g + 1]) = their node ids IN THE STACK, best first, in
 * the order of mlamg_gnn_topk (score descending under IEEE comparison, -0.0 == +0.0, then node
 * index ascending), so both are what mlamg_gnn_topk gives on the segment alone (idx + seg_ptr[g]):
 * that entry is this one on a single segment. One stable radix sort of (key, node index) pairs
 * over the stack (key: segment id, then score); its storage comes from a cached per-thread block,
 * and with the host mirrors given the call neither allocates (after the first of its size) nor
 * synchronises. Limits: 0 <= k_g <= n_g (n_g = 0 allowed), the stack has
 * fewer than 2^31 - 1 rows; the order of NaN scores is unspecified. EINVAL before any launch. */
int mlamg_gnn_topk_seg(const float* scores, const int64_t* seg_ptr, const int64_t* seg_ptr_host,
                       const int64_t* k_ptr, const int64_t* k_ptr_host, int64_t nb, float* vec,
                       int32_t* idx, void* stream);

/* A population stack (FullAggNet.forward_population: every individual of the genetic algorithm in
 * one pass): `members` equal copies of one base stack end to end. Member p owns rows
 * [p M, (p + 1) M) and edges [p E, (p + 1) E) (M, n, E below are PER MEMBER); node and edge ids in
 * src, tgt, tptr (members * n + 1 entries) and teid are ids of the whole stack; member p's tensor
 * of a parameter lies at ptr + p * pstride floats, one pstride for every weight argument of a
 * call (all parameters are views into one (members, total) matrix; pstride = 0: shared weights).
 * Member p's part of every output is bitwise what the single entry writes when run on that
 * member's rows or edges alone with member p's tensors: the single entries are these kernels
 * with members = 1, a workgroup works for one member, and no tile of rows or edges straddles two.
 * Limits, beyond the single entry's own (EINVAL before any launch, outputs untouched):
 * 1 <= members <= 65535, pstride >= 0, members * M, members * n and members * E < 2^31 - 1. */
/* mlamg_gnn_linear per member: W[N][K] and b[N] (nullable) are member-indexed. */
int mlamg_gnn_linear_pop(const float* X, int64_t M, int members, int K, const float* W,
                         const float* b, int64_t pstride, int N, int act, float beta,
                         const float* R, int rc, float* Y, void* stream);
/* mlamg_gnn_nnconv per member: L1, c1, L2, c2, L3, c3 and bias are member-indexed; root, R, Y
 * and msg_tmp[members * E * Fout] cover the whole stack. NULL tptr or X, or a NULL edge or
 * edge-network argument with E > 0, is refused too. */
int mlamg_gnn_nnconv_pop(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                         const float* ea, int64_t E, int members, int fe, const float* L1,
                         const float* c1, const float* L2, const float* c2, const float* L3,
                         const float* c3, int64_t pstride, const float* X, int64_t n, int Fin,
                         int Fout, const float* root, const float* bias, int act, const float* R,
                         int rc, float* msg_tmp, float* Y, void* stream);
/* mlamg_gnn_edge_mlp per member: W1, b1, g, beta, W2, b2 are member-indexed. With E > 0 no
 * argument but R may be NULL. */
int mlamg_gnn_edge_mlp_pop(const int32_t* src, const int32_t* tgt, const float* X, int F,
                           const float* ea, int fe, int64_t E, int members, const float* W1,
                           const float* b1, int H, const float* g, const float* beta,
                           const float* W2, const float* b2, int64_t pstride, int C, int act,
                           const float* R, int rc, float* out, void* stream);

/* The wide layers of ns/model/ali_interp.py InterpolationNetwork (ResidualBlock of TAGConv(K=5)
 * up to 256 channels, EdgeModel 513 -> 256 -> ... -> 1 with LayerNorms), fp32, device pointers
 * (csrc/gnn_wide.hip). Conventions as above: a size outside the limit stated at a prototype
 * returns MLAMG_EINVAL and writes nothing; every launch covers its whole index range. */
/* mlamg_gnn_linear's contract and epilogue on LDS tiles of the f32-input matrix cores
 * (v_mfma_f32_32x32x2_f32): every output's sum runs k = 0 .. K-1 in one accumulator chain from
 * +0.0 (no split-K), so Y is value-equal to mlamg_gnn_linear wherever both accept the shape (a
 * zero-padded k step can turn a -0.0 sum into +0.0). M == 0 returns without a launch.
 * Limits: 1 <= K <= 1024, 1 <= N <= 256, M >= 0, beta in {0, 1}, rc in {1, N} when R is given. */
int mlamg_gnn_linear_wide(const float* X, int64_t M, int K, const float* W, const float* b, int N,
                          int act, float beta, const float* R, int rc, float* Y, void* stream);
/* mlamg_gnn_propagate on wider rows: column f of Y is bitwise mlamg_gnn_propagate on column f of
 * X (the same edge-order fmaf chain). n == 0 returns without a launch. Limits: 1 <= F <= 256. */
int mlamg_gnn_propagate_wide(const int32_t* tptr, const int32_t* teid, const int32_t* src,
                             const float* w, const float* X, int64_t n, int F, float* Y,
                             void* stream);
/* torch LayerNorm over each row of X[rows][F] (biased variance, eps; weight and bias nullable:
 * 1 and 0), then + R[rows][F] (nullable), then act (0 none, 1 relu): EdgeModel.forward's order.
 * A wave per row; mean and variance are summed in double (lane l takes f = l, l + 64, ... in that
 * order, then the wave butterfly of csrc/reduce.hpp). rows == 0 returns without a launch.
 * Limits: 1 <= F <= 256, rows >= 0. */
int mlamg_gnn_layer_norm(const float* X, int64_t rows, int F, const float* weight,
                         const float* bias, float eps, const float* R, int act, float* Y,
                         void* stream);
/* The first EdgeModel block without the E x (2F + 1) concatenation: with U = X W[:, :F]^T and
 * V = X W[:, F:2F]^T (n x H each, two mlamg_gnn_linear_wide calls), per edge e
 *   h = ((U[src_e] + V[tgt_e]) + ea_e * w) + b,  out[e] = relu(LayerNorm(h) * g + beta)
 * (w[H] = W[:, 2F], LayerNorm as mlamg_gnn_layer_norm). E == 0 returns without a launch.
 * Limits: 1 <= H <= 256, E >= 0. */
int mlamg_gnn_edge_in(const int32_t* src, const int32_t* tgt, const float* U, const float* V,
                      const float* ea, int64_t E, int H, const float* w, const float* b,
                      const float* g, const float* beta, float eps, float* out, void* stream);
/* out[e] = |(v[e] - mean) / std| over the E values of v, std unbiased (torch.std's default,
 * ali_interp.py:174); mean and the squared deviations are summed in double in the fixed order
 * of csrc/reduce.hpp on a grid that depends on E alone. Limits: 2 <= E. */
int mlamg_gnn_standardize_abs(const float* v, int64_t E, float* out, void* stream);

/* greedy_coarsening (ns/lib/greedy.py:13-36) on HOST CSR arrays (csrc/greedy.cpp; touches no
 * device): rows whose dominance |a_ii| / sum_j |a_ij| reaches theta go to F in index order; then,
 * while undecided rows remain, the one of smallest dominance (ties: smallest index) goes to C
 * and each of its still undecided neighbours, in ascending index, has its dominance recomputed
 * over its undecided and F columns as they stand and moves to F at once if it reaches theta.
 * F[n], C[n] (capacity n each) receive the rows in the reference's append order, *nF and *nC
 * their counts. Sums are fp64 in ascending column order. EINVAL, before anything is written, on
 * a NULL argument, n < 0, rows that are not canonical (ascending, duplicate-free, in range), a
 * missing or zero diagonal, a non-finite value, or a NaN theta. Stored zeros off the diagonal are
 * no neighbours (scipy's nonzero() drops them). */
int mlamg_greedy_coarsening(int64_t n, const int32_t* indptr, const int32_t* indices,
                            const double* data, double theta, int32_t* F, int32_t* C,
                            int64_t* nF, int64_t* nC);

/* Seeded Bellman-Ford exactly as the reference's modified_bellman_ford (ns/lib/graph.py:7-53;
 * replaces that call at utils/evaluate_model.py:57, utils/evaluate_dataset.py:87): sweeps over
 * the edges (i -> j, weight g_ij rounded to fp32 like the torch COO values, ns/lib/sparse.py:28)
 * in row-major order, in place, `if d_i + g_ij < d_j: d_j = d_i + g_ij; nearest_j = nearest_i`
 * in fp32, until a sweep updates nothing. Run level-scheduled (csrc/graph.hip), so distances
 * AND nearest seeds, ties included, are bitwise the reference's. dist_f32[n] (+inf unreached),
 * nearest[n] (seed node id, -1 unreached: the reference leaves 0 there), *sweeps_host = the
 * reference's sweep count (the last one updates nothing). EINVAL on a negative self-loop or no
 * fixed point after n + 2 sweeps (the reference would never return). Syncs. */
int mlamg_bellman_ford(const mlamg_csr* G, const int32_t* seeds, int32_t k, float* dist_f32,
                       int32_t* nearest, int32_t* sweeps_host, void* stream);

/* Order-independent seeded Bellman-Ford (the multilevel / distributed hierarchy's aggregation,
 * which has no reference counterpart): the same fp32 distances (the order-independent fixed
 * point), label = smallest seed node id over tight in-edges; = mlamg_bellman_ford's labels
 * whenever shortest paths are unique. Multi-workgroup sweeps. *iters_host = synchronous sweeps. */
int mlamg_bellman_ford_canon(const mlamg_csr* G, const int32_t* seeds, int32_t k, float* dist_f32,
                             int32_t* cluster, int32_t* iters_host, void* stream);

/* mlamg_bellman_ford_canon taken apart, for the distributed setup (a sweep,
 * then the boundary (distance, label) exchange and an any-changed reduction, until no rank
 * changes anything; mlamg/dsetup.py). G may be a "global-shaped" operator whose rows outside a
 * rank's range are empty; every array is indexed by global node id.
 *   begin: w_f32[nnz] = (float)G.data, dist = +inf, cluster = INT32_MAX, is_seed = 0 for all n,
 *          then seeds[0..k): dist 0, cluster = itself, is_seed 1 (seeds may lie in any rank's
 *          range: every rank marks the global seed list);
 *   sweep: one push relaxation over G's rows (atomicMin; *changed = 1 if anything decreased —
 *          ghost copies included; the caller zeroes it);
 *   label: one min-label push along tight edges (dist final);
 *   end:   cluster INT32_MAX -> -1.
 * All asynchronous on `stream`. */
int mlamg_bf_canon_begin(const mlamg_csr* G, const int32_t* seeds, int32_t k, float* w_f32,
                         float* dist_f32, int32_t* cluster, int32_t* is_seed, void* stream);
int mlamg_bf_canon_sweep(const mlamg_csr* G, const float* w_f32, float* dist_f32, int32_t* changed,
                         void* stream);
int mlamg_bf_canon_label(const mlamg_csr* G, const float* w_f32, const float* dist_f32,
                         const int32_t* is_seed, int32_t* cluster, int32_t* changed, void* stream);
int mlamg_bf_canon_end(int32_t* cluster, int64_t n, void* stream);

/* pyamg 4.x graph.bellman_ford(G, seeds) exactly (the aggregation step of FullAggNet.forward,
 * ns/model/agg_interp.py:475; replaces that call): sequential in-place pull sweeps
 * x_i <- min(x_i, G_ij + x_j) over rows 0..n-1 in stored order, strict <, nearest seed from the
 * first strictly better neighbour, repeated until a sweep changes no distance; run
 * level-scheduled in one workgroup, so distances AND nearest seeds (ties included) are bitwise
 * pyamg's. Arithmetic in the graph's dtype: fp64 = 0 -> float32 (G's values must be exactly
 * representable, e.g. widened CNet weights; dist is float*), 1 -> float64 (dist is double*).
 * dist[n] (unreached: the dtype's max), nearest[n] (seed node id, -1 unreached), *sweeps_host =
 * pyamg's sweep count (the last one changes nothing). EINVAL if no fixed point after n + 2
 * sweeps (a negative cycle: pyamg would not return). Syncs. */
int mlamg_bellman_ford_pyamg(const mlamg_csr* G, const int32_t* seeds, int32_t k, int fp64,
                             void* dist, int32_t* nearest, int32_t* sweeps_host, void* stream);

/* The same sweep on a block-diagonal stack of nb graphs, one workgroup per graph: each walks the
 * level schedule of its own diagonal block and sweeps to its own fixed point, so per graph the
 * distances, the nearest seeds and the sweep count are bitwise mlamg_bellman_ford_pyamg on that
 * graph alone (nearest seeds as node ids in the stack). The two entries share the level rule,
 * the level bucketing and the sweep loop (csrc/graph.hip); they differ in how they launch it.
 *
 * plan_create reads G's pattern once on the host (the only host pass; syncs) and keeps, per
 * graph, its rows in level order and its level pointers. seg_ptr as in mlamg_gnn_*_seg above
 * (graphs of 0 rows allowed). EINVAL if seg_ptr does not cover G's rows, a graph has more than
 * 2^18 rows, or a stored entry couples two graphs (the message names the row).
 *
 * The run takes any G with the plan's pattern (n_rows and nnz are checked) and the seeds of
 * graph g in seeds[seed_ptr[g] .. seed_ptr[g + 1]) as node ids in the stack. dist / nearest /
 * fp64 as in mlamg_bellman_ford_pyamg; sweeps_host[nb] (nullable). A seed outside its own graph
 * is found on the device before anything is written: EINVAL, outputs untouched. A graph without
 * a fixed point after n_g + 2 sweeps (a negative cycle) gives EINVAL naming the first such graph;
 * the others' results are complete. Launches and the one read-back (2 nb + 1 words) do not depend
 * on nb. While it sweeps, a graph's distances and labels are kept in LDS when the largest graph's
 * fit in 64 KiB (8,192 rows in float32, 5,461 in float64; MLAMG_BF_SEG_LDS=0 keeps them in global
 * memory): same bits, 14-18 % faster. Syncs. */
typedef struct mlamg_bf_seg_plan mlamg_bf_seg_plan;
int mlamg_bellman_ford_pyamg_seg_plan_create(const mlamg_csr* G, const int64_t* seg_ptr,
                                             const int64_t* seg_ptr_host, int64_t nb,
                                             mlamg_bf_seg_plan** out, void* stream);
int mlamg_bellman_ford_pyamg_seg_plan_destroy(mlamg_bf_seg_plan* plan);
int mlamg_bellman_ford_pyamg_seg(const mlamg_bf_seg_plan* plan, const mlamg_csr* G,
                                 const int32_t* seeds, const int64_t* seed_ptr,
                                 const int64_t* seed_ptr_host, int fp64, void* dist,
                                 int32_t* nearest, int32_t* sweeps_host, void* stream);

/* out[0..k) (DEVICE int32) = np.random.RandomState(seed).permutation(n)[:k] bit for bit (numpy's
 * legacy MT19937 + Fisher-Yates; the seeds of ns/lib/graph.py:230-231 and
 * utils/evaluate_dataset.py:80-85): the draws on the host, the first k positions followed
 * through the swaps on the device (csrc/seeds.hip). Syncs. */
int mlamg_legacy_permutation(uint32_t seed, int64_t n, int64_t k, int32_t* out, void* stream);

/* Agg (n x k, values 1.0) from a per-node column assignment col[n] (-1 = no aggregate):
 * graph.py:56-86 nearest_center_to_agg and graph.py:234-238 AggOp. */
int mlamg_aggregate_op(const int32_t* col, int64_t n, int64_t k, mlamg_csr** out, void* stream);

/* map node-id labels to aggregate columns: col[i] = pos[label[i]] (graph.py:76-84). */
int mlamg_labels_to_columns(const int32_t* label, int64_t n, const int32_t* seeds, int32_t k,
                            int32_t* col, void* stream);

/* pyamg 4.x lloyd_cluster (called at ns/lib/graph.py:232 and behind
 * pyamg.aggregation.lloyd_aggregation, utils/common.py:91): up to maxiter rounds of {outward
 * Bellman-Ford, boundary detection, inward Bellman-Ford, recentre}, fp64 distances, the outward
 * pass in amg_core's sequential sweep order (as restated from pyamg 4.x's published source:
 * pyamg is absent here, so agreement with amg_core itself, ties included, is parity unpinned;
 * the device is bitwise the oracle's restatement, oracle/oracle.c lloyd_cluster). seeds (DEVICE, k) updated in place; dist[n], cluster[n] (aggregate index,
 * -1 none); *iters_host = rounds run (stops early when no seed moves). Syncs. */
int mlamg_lloyd_cluster(const mlamg_csr* G, int32_t* seeds, int32_t k, int maxiter, double* dist,
                        int32_t* cluster, int32_t* iters_host, void* stream);

/* The same with the order-independent label rule (min cluster index over tight pull
 * neighbours) and multi-workgroup sweeps: the hierarchy's Lloyd option. */
int mlamg_lloyd_cluster_canon(const mlamg_csr* G, int32_t* seeds, int32_t k, int maxiter,
                              double* dist, int32_t* cluster, int32_t* iters_host, void* stream);

/* ---------------------------------------------------------------- pyamg smoothed aggregation
 * Setup kernels of pyamg.aggregation.smoothed_aggregation_solver with its defaults, the
 * hierarchy the reference's PyAMG preconditioner builds (ns/preconditioner/PyAMG.py:94). pyamg is
 * absent: restated from its published algorithm (amg_core), parity unpinned; bitwise the
 * oracle's restatement (oracle/oracle.c pyamg_*). csrc/sa.hip.
 * symmetric_strength_of_connection(A, theta): row i keeps its diagonal and a_ij with
 * a_ij^2 >= theta^2 |a_ii| |a_jj| (stored order), values |a_ij| / (row max). */
int mlamg_symmetric_strength(const mlamg_csr* A, double theta, mlamg_csr** out, void* stream);
/* standard_aggregation(C) (amg_core, three greedy passes in row order; pass 1 decided in
 * parallel rounds, bitwise the sequential result): agg[n] (DEVICE) = aggregate of each row, -1
 * unaggregated; cpts (DEVICE, n, may be NULL) = the root of each aggregate; *n_agg = aggregates;
 * *rounds_host = pass-1 rounds. Syncs. */
int mlamg_standard_aggregation(const mlamg_csr* C, int32_t* agg, int32_t* cpts, int64_t* n_agg,
                               int32_t* rounds_host, void* stream);
/* fit_candidates(AggOp, B, tol) with one candidate: per aggregate (rows ascending)
 * norm = sqrt(sum B_i^2), T_i = B_i * (1 / norm) (0 if norm <= tol * norm), Bc = norm; T has
 * AggOp's pattern. B (DEVICE, n), Bc (DEVICE, n_agg). */
int mlamg_fit_candidates(const mlamg_csr* AggOp, const double* B, double tol, mlamg_csr** T_out,
                         double* Bc, void* stream);
/* C = A - B with scipy's csr binop rules (a - b, a - 0, 0 - b; zero results not stored), columns
 * ascending (jacobi_prolongation_smoother's P = T - D^-1 A T). */
int mlamg_csr_sub(const mlamg_csr* A, const mlamg_csr* B, mlamg_csr** out, void* stream);
/* pyamg get_diagonal(A, inv=True): dinv_i = 1 / (sum of row i's diagonal entries), 0 where that
 * sum is 0 (DEVICE, n). */
int mlamg_diag_pinv(const mlamg_csr* A, double* dinv, void* stream);

/* ---------------------------------------------------------------- Gauss-Seidel
 * pyamg relaxation.gauss_seidel (forward lexicographic, in place) used by the reference driver
 * (ns/lib/multigrid.py:175,184). Exact lexicographic order via level scheduling of the row
 * dependency DAG: bitwise identical to the sequential sweep. */
int mlamg_gs_create(const mlamg_csr* A, mlamg_gs** out, void* stream);
/* the same with a sweep direction (0 forward, 1 backward, 2 symmetric: forward then backward per
 * iteration) and block = 1 for pyamg relaxation.block_gauss_seidel's arithmetic with 1 x 1 blocks
 * (rsum = b_i - (0 + a_ij x_j) ..., x_i = 0 + Dinv_i rsum, Dinv_i = 1/a_ii or 0): the smoother and
 * the candidate improvement of pyamg.aggregation.smoothed_aggregation_solver
 * (ns/preconditioner/PyAMG.py:94; pyamg absent: parity unpinned, bitwise the oracle's
 * restatement, oracle/oracle.c pyamg_block_gauss_seidel) */
int mlamg_gs_create_ex(const mlamg_csr* A, int sweep, int block, mlamg_gs** out, void* stream);
int mlamg_gs_destroy(mlamg_gs* G);
int mlamg_gs_levels(const mlamg_gs* G, int32_t* n_levels);
int mlamg_gs_sweep(const mlamg_gs* G, double* x, const double* b, int iterations, void* stream);
/* The same sweeps on a block of k right-hand sides (multivectors as in the multi-vector section
 * below: fp64, row-major n x k, ld >= k, 1 <= k <= MLAMG_MV_MAX, 8-byte-aligned pointers, odd ld
 * allowed), X swept in place: the level schedule is walked once for all k columns. COLUMN j OF X
 * IS BITWISE mlamg_gs_sweep ON COLUMN j, for every handle mlamg_gs_create / _create_ex makes
 * (forward, backward, symmetric; gauss_seidel and block_gauss_seidel arithmetic): the smoother of
 * the reference driver (ns/lib/multigrid.py:175,184) and of pyamg's smoothed-aggregation solver
 * (ns/preconditioner/PyAMG.py:94) on a block. B may be NULL: every b_i is +0.0. B != X. NULL
 * arguments, k out of range, ld < k and B == X return MLAMG_EINVAL before any device call. */
int mlamg_gs_sweep_mv(const mlamg_gs* G, double* X, int64_t ldx, const double* B, int64_t ldb,
                      int k, int iterations, void* stream);
/* which kernels mlamg_gs_sweep_mv runs for k columns on G's (forward) schedule, a host function
 * of (G, k): 0 = one launch per level, 1 = one-workgroup walk on the CSR arrays, 2 = one-workgroup
 * walk on the level-ordered packed copy (csrc/gs_mv.hip) */
int mlamg_gs_mv_path(const mlamg_gs* G, int k, int32_t* path);
/* which kernel mlamg_gs_sweep runs, decided once at create (csrc/gs_plan.cpp): which = 0 for G's
 * own schedule, 1 for the backward schedule of a symmetric handle (MLAMG_EINVAL without one).
 * 0 LEVELS (one launch per level), 1 WORKGROUP (one workgroup on the CSR arrays), 2 WAVE (lanes
 * share a long row), 3 WRING (long rows, LDS ring), 4 PIPE (packed rows, pipelined), 5 PIPE_LDS
 * (the same with x in LDS), 6 RING (packed rows, LDS ring), 7 WINDOW (one-wave windowed sweep).
 * NULL arguments and which outside 0..1 return MLAMG_EINVAL before G is read. */
int mlamg_gs_path(const mlamg_gs* G, int which, int32_t* path);

/* ---------------------------------------------------------------- polynomial smoother
 * pyamg relaxation.polynomial(A, x, b, coefficients, iterations) (pyamg absent: parity unpinned,
 * the arithmetic is restated in DESIGN.md §32), the sweep behind presmoother=('chebyshev', ...).
 * coeffs_host (HOST, n_coeffs >= 1 finite numbers) in pyamg's order, coeffs[0] on the highest
 * power: what smoothing.setup_chebyshev keeps, -chebyshev_polynomial_coefficients(...)[:-1].
 * A (square) must outlive the handle; the handle owns three device vectors of A's size (r and two
 * h). A non-square A, n_coeffs < 1 and a non-finite coefficient return MLAMG_EINVAL before any
 * device call. */
int mlamg_poly_create(const mlamg_csr* A, const double* coeffs_host, int n_coeffs,
                      mlamg_poly** out, void* stream);
int mlamg_poly_destroy(mlamg_poly* S);
/* rows of the operator and the number of coefficients (each nullable) */
int mlamg_poly_info(const mlamg_poly* S, int64_t* rows, int* n_coeffs);
/* `iterations` times, in place on x (DEVICE): r = b - A x; h = c[0] r; h = c[i] r + A h for
 * i = 1 .. m-1; x = x + h, every multiply and add rounded on its own and A h the row sum of A's
 * active storage format (mlamg_spmv's): bitwise relaxation.polynomial in the formats that sum in
 * scipy's order. Costs m SpMV launches and m passes over A per iteration and nothing else: r and
 * c[0] r leave the first launch together, the last one adds into x (m = 1: one launch and a
 * copy). b NULL: a zero right-hand side. x_is_zero != 0: x is not read and counts as all +0.0 (the
 * same bits as the general path on such an x; for finite A), which turns the first pass over A
 * into one elementwise launch. No host synchronisation; b != x. */
int mlamg_poly_sweep(const mlamg_poly* S, double* x, const double* b, int iterations,
                     int x_is_zero, void* stream);
/* The same sweep on a block of k right-hand sides (multivectors as in the multi-vector section
 * below: row-major n x k, ld >= k, 1 <= k <= MLAMG_MV_MAX), X in place, the matrix stream read
 * once for all k columns per pass. COLUMN j OF X IS BITWISE mlamg_poly_sweep ON COLUMN j: in
 * scipy's order, or in the canonical CSR-vector order while A is in the VECTOR format. The k-wide
 * work space belongs to the handle and grows on demand, never inside a stream capture
 * (MLAMG_EINVAL there: sweep once at that width before capturing). B may be NULL; B != X. */
int mlamg_poly_sweep_mv(const mlamg_poly* S, double* X, int64_t ldx, const double* B, int64_t ldb,
                        int k, int iterations, int x_is_zero, void* stream);

/* ---------------------------------------------------------------- coarse direct solve
 * Replaces spla.factorized/splu (multigrid.py:168; MLAMG.py:122): the coarse operator is
 * inverted densely on the device (Gauss-Jordan, partial pivoting, fp64) once; each solve is a
 * dense GEMV. Returns MLAMG_EINVAL if the matrix is numerically singular. */
int mlamg_dense_create(const mlamg_csr* A, mlamg_dense** out, void* stream);
int mlamg_dense_destroy(mlamg_dense* D);
/* a given n x n row-major matrix M (host) applied as x = M b: the 'pinv' coarse solver of
 * pyamg's multilevel solver (M = scipy.linalg.pinv(A_c), formed by the caller as pyamg does;
 * ns/preconditioner/PyAMG.py:94). Syncs. */
int mlamg_dense_create_matrix(const double* M_host, int64_t n, mlamg_dense** out, void* stream);
/* which inverse was built: 1 = inverse Cholesky factor X = L^-1 with A^-1 = X^T X formed
 * (symmetric positive definite), 2 = the same factor kept and applied as X^T (X b), two
 * triangular passes (SPD operators of >= 2048 rows: no O(n^3) product), 0 = Gauss-Jordan with
 * partial pivoting (any other nonsingular operator) */
int mlamg_dense_info(const mlamg_dense* D, int* method, int64_t* n);
/* x = A^-1 b (device vectors), async on the stream. NOT reentrant on one handle: method 2 keeps
 * its intermediate X b in the handle's own buffer, so two solves with the same handle must be
 * ordered (same stream, or synchronised); use one handle per concurrent stream. */
int mlamg_dense_solve(const mlamg_dense* D, const double* b, double* x, void* stream);

/* Least squares by LSQR: x = argmin ||A x - b||_2 from x0 = 0, scipy.sparse.linalg.lsqr
 * semantics with damp = 0 (its defaults: atol = btol = 1e-6, conlim = 1e8, iter_lim <= 0 means
 * 2 * n_cols). Replaces spla.lsqr(P.T@A@P, P.T@(b - A@x))[0], the singular (Neumann) coarse solve
 * of ns/lib/multigrid.py:178-179. AT is A's explicit transpose (mlamg_transpose), the operator of
 * scipy's rmatvec. b (n_rows) and x (n_cols) are device vectors; the iteration runs on the device
 * (scalar recurrences in one thread, stop test on the device); synchronizes `stream`. istop_out /
 * itn_out (nullable): scipy's istop code (0..7) and iteration count. */
int mlamg_lsqr(const mlamg_csr* A, const mlamg_csr* AT, const double* b, double* x, double atol,
               double btol, double conlim, int iter_lim, int* istop_out, int* itn_out,
               void* stream);

/* x -= mean(x) (device vector; fixed-order sum / n): the nullspace normalisation of the singular
 * cycle, ns/lib/multigrid.py:186-187. */
int mlamg_remove_mean(double* x, int64_t n, void* stream);

/* ---------------------------------------------------------------- V-cycle executor
 * Multilevel weighted-Jacobi V(nu1,nu2) cycle: the two-level cycle of MLAMG.py:189-195 applied
 * recursively (the multilevel solver the PyAMG PC runs, PyAMG.py:94,119), coarsest level solved
 * with mlamg_dense. Levels are added fine to coarse; the hierarchy keeps references to the
 * handles (caller keeps them alive). */
int mlamg_hier_create(mlamg_hier** out);
int mlamg_hier_destroy(mlamg_hier* H);
/* level l: A, dinv_w (device, n), P (n x n_next), R = P^T */
int mlamg_hier_add_level(mlamg_hier* H, const mlamg_csr* A, const double* dinv_w,
                         const mlamg_csr* P, const mlamg_csr* R);
int mlamg_hier_set_coarse(mlamg_hier* H, const mlamg_csr* A_coarse, const mlamg_dense* D);
int mlamg_hier_set_smoothing(mlamg_hier* H, int nu_pre, int nu_post);
/* Stop-flag test of the cycle kernels (no reference counterpart; an A/B switch): 0 (default) =
 * tested only when mlamg_hier_vcycle has a tolerance (tol >= 0; without one nothing can raise
 * it, so the fixed-count cycles skip the per-kernel load); 1 = tested by every launch. */
int mlamg_hier_set_done_check(mlamg_hier* H, int always);
/* Opt-in factored prolongation at `level` (VERDICT r04 Next #5; not bitwise the explicit P):
 * x += t - dinv_w .* (A t), t = Agg e (t_i = e[agg[i]], 0 where agg[i] < 0), i.e. x += P e for
 * the SA prolongator P = (I - w D^-1 A) Agg without streaming P. A_uni: the level's operator in
 * the uniform row-pair format (EUNSUPPORTED otherwise; dinv_w = w / a_ii may be attached to it
 * with mlamg_csr_attach_dinv); agg (DEVICE, n) the aggregate column of each row; NULL A_uni
 * restores x += P e. */
int mlamg_hier_set_factored_prolong(mlamg_hier* H, int level, const mlamg_csr* A_uni,
                                    const int32_t* agg, const double* dinv_w);
/* smoother of one level: a Gauss-Seidel handle built on that level's operator (pyamg forward
 * sweep, in place; ns/lib/multigrid.py:175,184 — the reference amg_2_v), or NULL for weighted
 * Jacobi (default) */
int mlamg_hier_set_level_smoother(mlamg_hier* H, int level, const mlamg_gs* gs);
/* smoother of one level: a polynomial handle built on that level's operator (pyamg's
 * presmoother = postsmoother = ('chebyshev', {'iterations': iterations})), or NULL for the
 * default. Each of the cycle's nu_pre / nu_post sweeps is then `iterations` (>= 1) iterations of
 * mlamg_poly_sweep, n_coeffs passes over A each; coarse levels pre-smooth from a known-zero
 * guess, and a residual the cycle already holds is not recomputed. A level has one smoother:
 * setting this clears a Gauss-Seidel handle and mlamg_hier_set_level_smoother clears this one.
 * Both the single and the block cycle take such levels (bitwise per column). */
int mlamg_hier_set_level_polynomial(mlamg_hier* H, int level, const mlamg_poly* S, int iterations);
/* Coarsest solve without a size cap (replaces spla.factorized / splu, ns/lib/multigrid.py:168,
 * MLAMG.py:122, where a dense inverse no longer fits): PCG on A (SPD) preconditioned by one
 * V-cycle of the inner hierarchy M (built on A, finalised), to ||b - A x|| <= rtol ||b||, at most
 * maxit iterations. A and M must outlive the solver. */
int mlamg_pcg_create(const mlamg_csr* A, mlamg_hier* M, double rtol, int maxit, mlamg_pcg** out);
int mlamg_pcg_destroy(mlamg_pcg* C);
/* x = A^-1 b (DEVICE vectors), async on the stream (polls its convergence flag) */
int mlamg_pcg_solve(mlamg_pcg* C, const double* b, double* x, void* stream);
/* iterations of the last solve, solves that stopped at maxit, total iterations, largest final
 * relative residual over all solves (each nullable); syncs */
int mlamg_pcg_stats(const mlamg_pcg* C, int32_t* last_iters, int32_t* not_converged,
                    int32_t* total_iters, double* max_rel_residual, void* stream);
/* solves ended by a breakdown (p.Ap <= 0, r.z <= 0 or a NaN residual: A or the preconditioner
 * not positive definite; the solve stops with the iterate it had); syncs */
int mlamg_pcg_breakdowns(const mlamg_pcg* C, int32_t* breakdowns, void* stream);
/* *symmetric = 1 when A is square and |a_ij - a_ji| <= rtol * max(|a_ii|, |a_jj|) for every
 * stored entry (a missing a_ji counts as 0; rtol = 0: exact symmetry); the PCG coarse solve is
 * only chosen for such operators. Syncs. */
int mlamg_csr_symmetric(const mlamg_csr* A, double rtol, int* symmetric, void* stream);
/* Preconditioned GMRES with one V-cycle of M (a finalised hierarchy built on A) as the
 * preconditioner — the Krylov acceleration of the reference's PyAMG PC apply,
 * `Amg.solve(b, tol=amg_rtol, accel='gmres')` (ns/preconditioner/PyAMG.py:119). Algorithm of
 * scipy.sparse.linalg.gmres: restarted (restart <= 0: 20), left-preconditioned MGS, Givens,
 * gh-8400 inner tolerance control, stop when ||b - A x||_2 <= rtol ||b||_2; at most maxiter
 * restart cycles (<= 0: 10 n). x (device) is the initial guess (x_is_zero: known to be 0) and
 * the result. *info = 0 converged, else maxiter; *inner_iters = Krylov steps taken;
 * presid_hist_host (nullable, hist_cap entries) receives the preconditioned residual estimate
 * / ||b|| of every step. Syncs. */
int mlamg_gmres(const mlamg_csr* A, mlamg_hier* M, const double* b, double* x, double rtol,
                int restart, int maxiter, int x_is_zero, int* info, int* inner_iters,
                double* presid_hist_host, int hist_cap, void* stream);
/* pyamg.krylov.gmres with its default Householder orthogonalisation (pyamg 4.x
 * _gmres_householder; the Krylov loop of ns/preconditioner/PyAMG.py:119, pyamg absent: parity
 * unpinned): left-preconditioned by one V-cycle of M from a zero guess, returns at once if
 * ||M(b - A x0)|| < tol ||b||, else one cycle of at most min(maxiter, n) steps (maxiter <= 0:
 * min(n, 40)) until the rotated residual estimate < tol ||M(b - A x0)||. *info = 0 converged
 * (final ||M(b - A x)|| below that), else the step count; resid_hist_host (may be NULL): the
 * preconditioned residual norms, initial and per step, and the final one. Syncs per step. */
int mlamg_gmres_householder(const mlamg_csr* A, mlamg_hier* M, const double* b, double* x,
                            double tol, int maxiter, int x_is_zero, int* info, int* inner_iters,
                            double* resid_hist_host, int hist_cap, void* stream);
/* use the PCG solver C (size = A_coarse rows) as H's coarsest solve instead of a dense inverse;
 * cycles of such a hierarchy run eagerly (use_graph is ignored) */
int mlamg_hier_set_coarse_pcg(mlamg_hier* H, const mlamg_csr* A_coarse, mlamg_pcg* C);
/* H's coarsest solve by restarted GMRES (mlamg_gmres's algorithm) on A_coarse, preconditioned by
 * one V-cycle of `inner` (a hierarchy of A_coarse, kept alive by the caller), from a zero guess
 * to ||b - A_c x|| <= rtol ||b|| (restart, maxiter restart cycles): for a coarse operator that is
 * not SPD (PCG does not apply) and beyond the dense inverse's size — the reference factors any
 * nonsingular A_H with SuperLU (ns/lib/multigrid.py:165-170). Cycles run eagerly. A solve that
 * ends above fail_rtol makes the cycle call return MLAMG_EINVAL ("did not converge"), as a
 * failed factorisation would. */
int mlamg_hier_set_coarse_gmres(mlamg_hier* H, const mlamg_csr* A_coarse, mlamg_hier* inner,
                                double rtol, double fail_rtol, int restart, int maxiter);
/* GMRES coarse-solve statistics since H was built: solves, steps of the last one, total steps,
 * solves that did not reach rtol, largest final relative residual (each nullable) */
int mlamg_hier_coarse_gmres_stats(const mlamg_hier* H, int32_t* solves, int32_t* last_iters,
                                  int32_t* total_iters, int32_t* not_converged,
                                  double* worst_rel);
/* ---------------------------------------------------------------- batched reference solves
 * The reference's own call pattern — two-level amg_2_v(A, P, b, x, ...) on small grids
 * (ns/lib/multigrid.py:111-210, called per grid by utils/common.py:77,106,
 * utils/evaluate_dataset.py:96, utils/train_dataset.py:114) — for a whole batch of problems in
 * ONE kernel launch, one workgroup per problem: Galerkin P^T A P, dense coarse inverse, every
 * cycle and the tolerance test on the device (csrc/batch.hip). All arrays are HOST memory (the
 * caller's scipy/numpy buffers); the call packs them, copies them in once, runs, copies the
 * results out and returns (synchronous on `stream`). Limits: mlamg_amg2v_batch_limits. */
typedef struct mlamg_amg2v_problem {
  int64_t n, n_c;                                          /* A is n x n, P is n x n_c */
  const int32_t* A_indptr; const int32_t* A_indices; const double* A_data; int64_t A_nnz;
  const int32_t* P_indptr; const int32_t* P_indices; const double* P_data; int64_t P_nnz;
  const double* b; const double* x0;                       /* length n */
  double* x_out;                                           /* length n */
  double* err_out;                                         /* length max_iter; err[:iters] written */
  int32_t iters_out;                                       /* len(err) */
  int32_t status_out;                                      /* 0 ok, 1 A_H exactly singular (x = x0,
                                                              iters 0: multigrid.py:167-170) */
} mlamg_amg2v_problem;
/* smoother 0 = pyamg forward Gauss-Seidel (the reference's), 1 = weighted Jacobi
 * x += w D^-1 (b - A x) (MLAMG.py:143-146 form, w = jacobi_weight); norm_mode 0 = res_tol
 * (||b - A x||_2), 1 = error_tol (||x||_2); stop after the first cycle with norm <= tol
 * (tol < 0: never). */
int mlamg_amg2v_batch(mlamg_amg2v_problem* probs, int count, int smoother, int nu_pre,
                      int nu_post, double jacobi_weight, int norm_mode, double tol, int max_iter,
                      void* stream);
/* largest n, n_c and off-diagonal entries per row of A the batched solver accepts */
int mlamg_amg2v_batch_limits(int64_t* max_rows, int64_t* max_coarse, int* max_row_entries);
/* what res_hist records each cycle: 0 = ||b - A x||_2 (default, MLAMG.py:194 / res_tol),
 * 1 = ||x||_2 (amg_2_v error_tol, multigrid.py:193); the tolerance test applies to it */
int mlamg_hier_set_norm(mlamg_hier* H, int mode);
/* run n_cycles V-cycles on (b, x) (x updated in place). After each cycle ||b - A x||_2 is
 * written to res_hist[c] (DEVICE, may be NULL). If tol >= 0 the cycle loop stops after the
 * first cycle with ||r|| <= tol (MLAMG.py:194; tol = 0 stops on an exactly zero norm, like the
 * reference's `e <= tol`); tol < 0 = no tolerance. *cycles_done_host (nullable) receives the count and
 * the call syncs. use_graph != 0 replays one captured hipGraph per cycle. */
/* b may be NULL: a zero right-hand side (every fine-level kernel takes b = +0.0 instead of
 * reading a vector of zeros; the same bits as an all-zero b). */
int mlamg_hier_vcycle(mlamg_hier* H, const double* b, double* x, int n_cycles, double tol,
                      double* res_hist, int32_t* cycles_done_host, int use_graph, void* stream);
/* bytes of one V-cycle with every operator priced as CSR (SURVEY.md §8(d) model): a
 * CSR-EQUIVALENT figure — re-encoded operators (rowpat, value codes) move far fewer bytes, so
 * this divided by the cycle time may exceed the HBM peak */
int mlamg_hier_cycle_bytes(const mlamg_hier* H, double* bytes);
/* bytes one V-cycle must move through HBM with every operator priced as the format it is stored
 * in (mlamg_csr_format_bytes per launch + the epilogues' vectors): the cycle's roofline bytes */
int mlamg_hier_cycle_format_bytes(const mlamg_hier* H, double* bytes);

/* ---------------------------------------------------------------- multi-vector (n x k) path
 * A multivector is fp64, row-major n x k with a leading dimension ld >= k counted in doubles
 * (a contiguous torch (n, k) tensor, or a column slice of a wider one; the layout of the
 * reference's test-vector block, ns/model/loss.py:59). 1 <= k <= MLAMG_MV_MAX. Pointers need
 * only be 8-byte aligned and ld may be odd (16-byte accesses are used where alignment allows).
 * Every row is summed per column left to right in stored order with separate multiply and add,
 * i.e. scipy's csr_matvecs: COLUMN j OF EVERY RESULT IS BITWISE THE SINGLE-VECTOR RESULT ON
 * COLUMN j. The kernels read the CSR arrays and the row-block table, which every exact format
 * keeps, so they do not depend on the format active on the handle; the matrix stream is read
 * once for all k columns. All entries are async on `stream`; NULL arguments, k out of range and
 * ld < k return MLAMG_EINVAL before any device call. */
#define MLAMG_MV_MAX 64

/* Y = alpha*A@X + beta*Y (X: n_cols x k, Y: n_rows x k). alpha==1 && beta==0 gives A@X bit for
 * bit per column (ns/model/loss.py:70,78 `A @ x` on an N x k block). */
int mlamg_spmm(const mlamg_csr* A, const double* X, int64_t ldx, double* Y, int64_t ldy, int k,
               double alpha, double beta, void* stream);

/* R = B - A@X. B may be NULL: a zero right-hand side taken as +0.0 (the bits of the single path).
 * norms (DEVICE, k doubles, nullable): ||R[:, j]||_2 in mlamg_norm2's order. */
int mlamg_residual_mv(const mlamg_csr* A, const double* B, int64_t ldb, const double* X,
                      int64_t ldx, double* R, int64_t ldr, int k, double* norms, void* stream);

/* nu weighted-Jacobi sweeps X += dinv_w .* (B - A@X) on every column (dinv_w: one vector of n,
 * shared; the two roundings of mlamg_jacobi: r = b - s; x + d*r). X_tmp: scratch n x k with
 * leading dimension ldt. Result lands in X. B may be NULL (zero right-hand side). */
int mlamg_jacobi_mv(const mlamg_csr* A, const double* dinv_w, const double* B, int64_t ldb,
                    double* X, int64_t ldx, double* X_tmp, int64_t ldt, int k, int nu,
                    void* stream);

/* Bc = R@Rf (mlamg_restrict per column) and X += P@E (mlamg_prolong_add per column). */
int mlamg_restrict_mv(const mlamg_csr* R, const double* Rf, int64_t ldr, double* Bc, int64_t ldb,
                      int k, void* stream);
int mlamg_prolong_add_mv(const mlamg_csr* P, const double* E, int64_t lde, double* X, int64_t ldx,
                         int k, void* stream);

/* The same four products with every row summed in the CANONICAL CSR-VECTOR ORDER instead of
 * scipy's (csrc/spmm_vec.hip; the order of the VECTOR format: 512 virtual lanes, entry e of a row
 * to lane e mod 512, an xor butterfly per 64 lanes, the eight wave sums added in order; restated
 * in oracle/oracle.c vec_matvec). COLUMN j OF EVERY RESULT IS BITWISE THE SINGLE-VECTOR ENTRY ON
 * COLUMN j WITH THE VECTOR FORMAT ACTIVE ON THE HANDLE, AT ANY WIDTH: mlamg_spmv (alpha and beta
 * as there; with beta == 0 Y is not read), mlamg_residual, mlamg_jacobi, mlamg_prolong_add; a
 * restriction is mlamg_spmm_vec(R, ..., 1, 0). The result does not depend on the handle's vector
 * width, on k, on leading dimensions or on pointer alignment. norms: as mlamg_residual_mv. The
 * entries read the CSR arrays (the 16-bit column copy of the VECTOR format where the handle has
 * one) and, like mlamg_spmm, do not require a particular active format: on a handle whose active
 * format is VECTOR these, not mlamg_spmm and its kin, give the bits of the single-vector
 * entries. Arguments and their checks as above; the message names the argument. */
int mlamg_spmm_vec(const mlamg_csr* A, const double* X, int64_t ldx, double* Y, int64_t ldy,
                   int k, double alpha, double beta, void* stream);
int mlamg_residual_mv_vec(const mlamg_csr* A, const double* B, int64_t ldb, const double* X,
                          int64_t ldx, double* R, int64_t ldr, int k, double* norms, void* stream);
int mlamg_jacobi_mv_vec(const mlamg_csr* A, const double* dinv_w, const double* B, int64_t ldb,
                        double* X, int64_t ldx, double* X_tmp, int64_t ldt, int k, int nu,
                        void* stream);
int mlamg_prolong_add_mv_vec(const mlamg_csr* P, const double* E, int64_t lde, double* X,
                             int64_t ldx, int k, void* stream);

/* out[j] (DEVICE, k doubles) = ||X[:, j]||_2, bitwise mlamg_norm2 of that column. */
int mlamg_norm2_mv(const double* X, int64_t ldx, int64_t n, int k, double* out, void* stream);

/* X[:, j] -= mean(X[:, j]), bitwise mlamg_remove_mean of that column. */
int mlamg_remove_mean_mv(double* X, int64_t ldx, int64_t n, int k, void* stream);

/* X = A_c^-1 B for the three mlamg_dense_info methods, per column bitwise mlamg_dense_solve; the
 * dense operator is read once for all k columns. Not reentrant on one handle (method 2). */
int mlamg_dense_solve_mv(const mlamg_dense* D, const double* B, int64_t ldb, double* X,
                         int64_t ldx, int k, void* stream);

/* ---- a batch of independent problems as one block-diagonal stack (mlamg/loss.py AmgLossBatch)
 * The rows of a stacked multivector are cut into nb consecutive segments, segment s the rows
 * [seg_offsets[s], seg_offsets[s + 1]) (DEVICE, nb + 1 int64 entries, ascending from 0); max_len
 * is the longest segment's length (a shorter value gives unspecified results, never an access
 * outside the segments). 1 <= nb <= 65535. All segments run in one launch per stage. NULL
 * arguments, k out of range, ld < k and nb out of range return MLAMG_EINVAL before any device
 * call; the message names the function and the argument. */

/* out[s * k + j] (DEVICE, nb x k doubles) = ||X[segment s, j]||_2. FOR EVERY SEGMENT BITWISE
 * mlamg_norm2_mv ON THAT SEGMENT'S ROWS ALONE: segment s keeps the single kernels' partition
 * (min(1024, ceil(n_s / 256)) row blocks walked with the same stride, partials summed in the same
 * order). */
int mlamg_norm2_seg_mv(const double* X, int64_t ldx, int k, const int64_t* seg_offsets,
                       int64_t nb, int64_t max_len, double* out, void* stream);

/* every segment's rows lose their own column means. FOR EVERY SEGMENT BITWISE
 * mlamg_remove_mean_mv ON THAT SEGMENT'S ROWS ALONE (the fixed 512 row blocks, the same order of
 * the partials, the mean divides by n_s; row blocks that own no rows contribute the +0.0 they
 * contribute there). */
int mlamg_remove_mean_seg_mv(double* X, int64_t ldx, int k, const int64_t* seg_offsets,
                             int64_t nb, int64_t max_len, void* stream);

/* The inverses of the nb diagonal blocks of the square CSR A_c, block b the rows and columns
 * [offsets_host[b], offsets_host[b + 1]) (HOST, nb + 1 entries from 0 to n). BLOCK b's INVERSE IS
 * BITWISE WHAT mlamg_dense_create BUILDS FOR THAT BLOCK ALONE, by the same rule per block: 64
 * rows or more try the inverse Cholesky factor first (method 1), smaller blocks and blocks that
 * fail its symmetry or pivot test take Gauss-Jordan with partial pivoting (method 0); the whole
 * batch is inverted in a handful of launches whatever nb is (csrc/blockdense.hip). MLAMG_EINVAL,
 * with a message naming the row / the block: an entry outside the diagonal blocks (the first
 * such row), a block at or above mlamg_dense_create's method-2 threshold (2048 rows; the batch
 * is for small coarse problems), an exactly singular block. Syncs. */
int mlamg_blockdense_create(const mlamg_csr* A_c, const int64_t* offsets_host, int64_t nb,
                            mlamg_blockdense** out, void* stream);
int mlamg_blockdense_destroy(mlamg_blockdense* D);
/* nb, the stacked rows n and methods[b] (HOST, nb ints) = mlamg_dense_info's method of block b;
 * every output is nullable */
int mlamg_blockdense_info(const mlamg_blockdense* D, int64_t* nb, int64_t* n, int* methods);
/* X_b = inv_b B_b for every block in one launch (B, X: stacked n x k multivectors). EVERY BLOCK'S
 * ROWS ARE BITWISE mlamg_dense_solve_mv OF A HANDLE CREATED ON THAT BLOCK ALONE. B != X. */
int mlamg_blockdense_solve_mv(const mlamg_blockdense* D, const double* B, int64_t ldb, double* X,
                              int64_t ldx, int k, void* stream);

/* n_cycles V(nu1,nu2) cycles of a finalised hierarchy on the block (B, X), X updated in place:
 * the step sequence of mlamg_hier_vcycle on every column, hence its bits. B may be NULL (zero
 * right-hand side). remove_mean != 0 subtracts each column's mean after the post-smoothing of
 * every cycle (ns/model/loss.py:89; ns/lib/multigrid.py:186-187). hist (DEVICE, n_cycles x k
 * row-major, nullable) receives after each cycle, per column, ||b - A x||_2 (norm_mode 0) or
 * ||x||_2 (norm_mode 1), taken after the mean removal. A fixed cycle count (no tolerance stop),
 * run eagerly. The coarsest solve is the dense inverse (mlamg_dense_solve_mv) or the block PCG
 * (mlamg_pcg_solve_mv; a breakdown is counted in the solver's statistics, not returned).
 * MLAMG_EUNSUPPORTED for a Gauss-Seidel level smoother (unless the hierarchy asked for it:
 * mlamg_hier_set_mv_gauss_seidel), a GMRES coarse solve, a factored prolongation, or any operator
 * in the VECTOR format (unless the hierarchy asked for it: mlamg_hier_set_mv_vector). */
int mlamg_hier_vcycle_mv(mlamg_hier* H, const double* B, int64_t ldb, double* X, int64_t ldx,
                         int k, int n_cycles, int norm_mode, int remove_mean, double* hist,
                         void* stream);
/* on != 0: mlamg_hier_vcycle_mv takes Gauss-Seidel levels (mlamg_hier_set_level_smoother) through
 * mlamg_gs_sweep_mv, mirroring the single cycle's steps (a coarse Gauss-Seidel level sweeps a
 * zeroed iterate block in place; the finest sweeps X in place), so column j keeps the bits of
 * mlamg_hier_vcycle on column j: the reference driver's amg_2_v smoother
 * (ns/lib/multigrid.py:175,184) and pyamg's symmetric block Gauss-Seidel on every level
 * (ns/preconditioner/PyAMG.py:94) on a block of right-hand sides. Jacobi and Gauss-Seidel levels
 * may mix. Default 0: such a hierarchy is refused as before. A Krylov solver's inner hierarchy
 * (mlamg_pcg_solve_mv) stays weighted-Jacobi only. */
int mlamg_hier_set_mv_gauss_seidel(mlamg_hier* H, int on);
/* on != 0: mlamg_hier_vcycle_mv takes operators in the VECTOR format (which the family rule of
 * mlamg_hier_apply_formats gives every long-row coarse operator). Each launch of the block cycle
 * then follows its own operator: the canonical-order kernel (mlamg_spmm_vec and its kin) for an
 * operator whose format is VECTOR, the scipy-order kernel for every other one, so column j keeps
 * the bits of mlamg_hier_vcycle on column j. Formats may mix within a level; composes with
 * mlamg_hier_set_mv_gauss_seidel and with a PCG coarse solve. Default 0: such a hierarchy is
 * refused as before. A Krylov solver's inner hierarchy (mlamg_pcg_solve_mv) keeps refusing. */
int mlamg_hier_set_mv_vector(mlamg_hier* H, int on);

/* X = A^-1 B by PCG on the n_c x k block (B, X) (multivectors as above; B != X): the iteration
 * of mlamg_pcg_solve on every column at once, the operator and the preconditioner's hierarchy
 * streamed once per iteration for all k columns. COLUMN j OF X AND COLUMN j'S ITERATION COUNT
 * ARE BITWISE WHAT mlamg_pcg_solve GIVES ON COLUMN j ALONE: every dot product keeps the single
 * kernel's partition and summation order per column, and the updates round as the single
 * kernels do. Each column has its own scalars, done flag and iteration counter; a column that
 * has converged, has a zero right-hand side or broke down (p.Ap <= 0, r.z <= 0 or a NaN) is
 * frozen (its x, r and p are no longer written) while the others continue. The host polls an
 * all-columns-done flag as mlamg_pcg_solve polls its done flag; inside a stream capture all
 * maxit iterations are recorded. The cumulative statistics (mlamg_pcg_stats,
 * mlamg_pcg_breakdowns) afterwards read as after k single solves, column 0 first. The n_c x k
 * work blocks are owned by the solver and grown on demand (not capture-safe on first use of a
 * larger k). MLAMG_EUNSUPPORTED where the preconditioner's hierarchy has no block cycle (see
 * mlamg_hier_vcycle_mv; its coarsest solve must be dense). Not reentrant on one solver. The
 * solver's own A p product is summed in scipy's order whatever A's format: on an A in the VECTOR
 * format the columns are not the bits of mlamg_pcg_solve (hierarchies set up through
 * mlamg/hierarchy.py never put a PCG operator there). */
int mlamg_pcg_solve_mv(mlamg_pcg* C, const double* B, int64_t ldb, double* X, int64_t ldx, int k,
                       void* stream);
/* iters[j] (HOST, k entries) = iterations column j took in the last mlamg_pcg_solve_mv (k at
 * most that call's k); syncs */
int mlamg_pcg_iters_mv(const mlamg_pcg* C, int32_t* iters, int k, void* stream);

/* mlamg_gmres on the n x k block (B, X) (multivectors as above; B != X): the restarted MGS GMRES
 * of mlamg_gmres run in lock-step on every column, so that each inner step applies the operator
 * (one SpMM), the preconditioner (one zero-guess block cycle of M) and every Gram-Schmidt dot and
 * update once for all k columns. COLUMN j OF X, info[j], inner_iters[j] AND COLUMN j OF THE HISTORY
 * ARE BITWISE WHAT mlamg_gmres RETURNS ON COLUMN j ALONE with the same rtol, restart, maxiter and
 * x_is_zero: every dot keeps the single kernels' partition and order per column, and each column
 * has its own Hessenberg columns, rotations, status, ptol and ||b||. A column whose inner stop
 * fires is frozen for the rest of that restart cycle; one that has converged, has ||b|| = 0
 * (x = b, 0 steps, info 0), starts below rtol ||b|| or broke down is frozen for good (its x is no
 * longer written) while the others continue; the solve ends when no column is left or after
 * maxiter restart cycles. X (device) holds the initial guesses (x_is_zero: known to be 0) and the
 * results. info, inner_iters: HOST, k entries. presid_hist_host (HOST, nullable): hist_cap x k
 * row-major, column j receives the preconditioned residual estimate / ||b_j|| of its first
 * min(inner_iters[j], hist_cap) steps. M's block cycle takes what mlamg_hier_vcycle_mv takes: a
 * dense or a PCG coarse solve, Gauss-Seidel levels after mlamg_hier_set_mv_gauss_seidel, VECTOR
 * operators after mlamg_hier_set_mv_vector (A in the VECTOR format is then summed in the canonical
 * order, as mlamg_gmres sums it); MLAMG_EUNSUPPORTED otherwise, and for a GMRES coarse solve or a
 * factored prolongation. The (restart + 1) n x k Krylov blocks live in M's Krylov workspace.
 * NULL arguments, k out of range, ld < k and B == X return MLAMG_EINVAL before any device call.
 * Syncs; not capturable. */
int mlamg_gmres_mv(const mlamg_csr* A, mlamg_hier* M, const double* B, int64_t ldb, double* X,
                   int64_t ldx, int k, double rtol, int restart, int maxiter, int x_is_zero,
                   int32_t* info, int32_t* inner_iters, double* presid_hist_host, int hist_cap,
                   void* stream);

/* Sampled dense-dense product on S's pattern (csrc/sddmm.hip; the gradient of amg_loss with
 * respect to a prolongator's stored values, mlamg/loss.py):
 *   out[e] = alpha * sum_{c<k} U[row(e), c] * V[col(e), c] + beta * out[e]
 * for every stored entry e of S, in S's CSR entry order (out: nnz doubles; S's values are not
 * read). U is n_rows x k and V is n_cols x k, multivectors as above (ldu, ldv >= k). With
 * beta == 0 out is not read. The kernel reads S's CSR arrays and row-block table only, so it
 * does not depend on the format active on the handle.
 * SUMMATION ORDER, a fixed function of k: with G the smallest power of two >= ceil(k/2) and the
 * columns k .. 2G-1 of U and V taken as +0.0,
 *   t[p] = (U[i,2p] * V[j,2p]) + (U[i,2p+1] * V[j,2p+1]),  p = 0 .. G-1,
 * then t[q] = t[2q] + t[2q+1] (q = 0 .. len/2-1) until one term s is left, and
 *   out = alpha * s (beta == 0) or (alpha * s) + (beta * out),
 * every multiply and add rounded on its own. It does not depend on the row-block partition, the
 * entry's position in its row, ldu / ldv, pointer alignment or the (16-byte or 8-byte access)
 * instantiation that ran. */
int mlamg_sddmm(const mlamg_csr* S, const double* U, int64_t ldu, const double* V, int64_t ldv,
                int k, double alpha, double beta, double* out, void* stream);

/* ---------------------------------------------------------------- multi-GPU (RCCL over xGMI)
 * New relative to the reference, whose only parallelism is a process task farm over independent
 * grids (ns/parallel/pool.py:139-186, pickled objects over pipes / mpi4py, no collectives).
 * One process per GPU; the fine level is row-partitioned, coarse levels replicated
 * (SURVEY.md §8e). The unique id (128 bytes) is created on rank 0 and broadcast by the caller. */
typedef struct mlamg_halo mlamg_halo;
typedef struct mlamg_dhier mlamg_dhier;
int mlamg_comm_unique_id(void* id_out);
int mlamg_comm_create(const void* id, int nranks, int rank, mlamg_comm** out);
int mlamg_comm_destroy(mlamg_comm* c);
/* the communicator's size, rank and device as the transport reports them (RCCL:
 * ncclCommCount / ncclCommUserRank / ncclCommCuDevice); transport_out (nullable): 0 = RCCL,
 * 1 = loopback, 2 = null (timing only). device_out nullable. */
int mlamg_comm_info(const mlamg_comm* c, int* nranks_out, int* rank_out, int* device_out,
                    int* transport_out);
/* In-process test transport (RCCL refuses two ranks on one GPU): the ranks of a loop group are
 * host threads of ONE process, each with its own stream on the same device; send/recv become
 * device-to-device copies ordered by events, the all-reduce sums in rank order. Same message
 * order as the RCCL calls it stands in for; not capturable into a graph. For testing the
 * distributed executor at world sizes > 1 on a single GPU. */
typedef struct mlamg_loop_group mlamg_loop_group;
int mlamg_loop_group_create(int nranks, mlamg_loop_group** out);
int mlamg_loop_group_destroy(mlamg_loop_group* g);
int mlamg_comm_create_loopback(mlamg_loop_group* g, int rank, mlamg_comm** out);
/* Timing-only communicator: rank `rank` of `nranks` whose exchanges (halos, allgather,
 * all-reduce) are skipped — ghost values and norms are NOT exchanged, results are invalid. It
 * measures one rank's device work (kernels, packs) of the distributed cycle on one GPU. */
int mlamg_comm_create_null(int nranks, int rank, mlamg_comm** out);
int mlamg_comm_allreduce_sum(mlamg_comm* c, double* buf, int64_t n, void* stream);
/* ghost layout of one rank: x_ext = [owned n_own | ghosts]; for neighbour q (ascending),
 * send_cnt[q] owned entries (send_idx_host, concatenated) and recv_cnt[q] ghosts, stored
 * contiguously in neighbour order. */
int mlamg_halo_create(mlamg_comm* c, int64_t n_own, int32_t n_nbr, const int32_t* nbr,
                      const int64_t* send_cnt, const int32_t* send_idx_host,
                      const int64_t* recv_cnt, mlamg_halo** out);
int mlamg_halo_destroy(mlamg_halo* h);
int mlamg_halo_exchange(mlamg_halo* h, double* x_ext, void* stream);
/* partitioned V-cycle over the first K levels (mlamg/partition.py build_levels):
 * coarse = hierarchy of the replicated levels K..L, nc = its size, c_lo_all/c_hi_all = every
 * rank's owned segment of that space (they tile [0, nc) in rank order). Then add levels fine to
 * coarse: A_loc (n_own x n_own+ghosts_x), R_own (owned next-level rows x n_own+ghosts_r), P_loc
 * (n_own x next own+ghosts_p with halo_p) — or, on the last partitioned level, P_loc with the
 * replicated coarse columns and halo_p = NULL. The cycle iterates on x_ext (owned part first). */
int mlamg_dhier_create(mlamg_comm* c, mlamg_hier* coarse, int64_t nc, const int64_t* c_lo_all,
                       const int64_t* c_hi_all, mlamg_dhier** out);
int mlamg_dhier_add_level(mlamg_dhier* D, const mlamg_csr* A_loc, const double* dinv_w,
                          const mlamg_csr* P_loc, const mlamg_csr* R_own, mlamg_halo* halo_x,
                          mlamg_halo* halo_r, mlamg_halo* halo_p);
int mlamg_dhier_destroy(mlamg_dhier* D);
/* halo / interior overlap (SURVEY.md §8e "overlapped with the interior SpMV"): operator `which`
 * (0 = A_loc behind halo_x, 1 = R_own behind halo_r, 2 = P_loc behind halo_p) of `level` given
 * as three consecutive row blocks lo | mid | hi (lo, hi may be NULL; each starts on an even row;
 * same columns as the operator) where mid reads no ghost entry. The cycle then posts the
 * exchange on a stream of its own and runs mid meanwhile, lo and hi after it; every row is
 * summed as in the unsplit operator (exact-order formats), so the iterate is unchanged. Call
 * before the first cycle. */
int mlamg_dhier_set_split(mlamg_dhier* D, int level, int which, const mlamg_csr* lo,
                          const mlamg_csr* mid, const mlamg_csr* hi);
/* use the splits (default 1) or run every exchange before its whole operator (0) */
int mlamg_dhier_set_overlap(mlamg_dhier* D, int on);
int mlamg_dhier_set_coarse_graph(mlamg_dhier* D, int use_graph);
/* capture one whole distributed cycle (kernels and RCCL send/recv/all-reduce) into a hipGraph
 * and replay it (default off); re-captured when b, x, res_hist, tol or a kernel format change */
int mlamg_dhier_set_cycle_graph(mlamg_dhier* D, int use_graph);
/* b may be NULL: this rank's part of the right-hand side is zero (as mlamg_hier_vcycle) */
int mlamg_dhier_vcycle(mlamg_dhier* D, const double* b, double* x_ext, int n_cycles, double tol,
                       double* res_hist, int32_t* cycles_done_host, void* stream);

/* ---------------------------------------------------------------- boundary-contract spellings
 * The entry points as the drop-in contract names them, thin forms of the API
 * above (csrc/contract.hip). */
/* lloyd_cluster of ns/lib/graph.py:232 (pyamg 4.x): = mlamg_lloyd_cluster without the distance
 * output. seeds_inout, cluster_out on the DEVICE. Syncs. */
int mlamg_lloyd(const mlamg_csr* G, int32_t* seeds_inout, int32_t k, int maxiter,
                int32_t* cluster_out, void* stream);
/* n_cycles V-cycles (MLAMG.py:189-195 per level), ||b - A x||_2 per cycle into res_hist (DEVICE,
 * nullable), no tolerance stop, replayed from a captured hipGraph: = mlamg_hier_vcycle. */
int mlamg_vcycle(const mlamg_hier* H, const double* b, double* x, int n_cycles, double* res_hist,
                 void* stream);
/* process-default RCCL communicator (one per process; the id from mlamg_comm_unique_id on rank
 * 0, broadcast by the caller); mlamg_comm_default returns it, mlamg_comm_finalize frees it. */
int mlamg_comm_init(const void* nccl_unique_id, int nranks, int rank);
int mlamg_comm_default(mlamg_comm** out);
int mlamg_comm_finalize(void);
/* one rank's operator: n_own owned rows, columns renumbered into x_ext = [owned | n_ghost
 * ghosts] (mlamg/partition.py), plus its x halo on the default communicator (layout as in
 * mlamg_halo_create; recv counts must add up to n_ghost). */
int mlamg_csr_create_partitioned(int64_t n_own, int64_t n_ghost, int64_t nnz,
                                 const int32_t* indptr, const int32_t* indices,
                                 const double* data, int on_device, int32_t n_nbr,
                                 const int32_t* nbr, const int64_t* send_cnt,
                                 const int32_t* send_idx_host, const int64_t* recv_cnt,
                                 mlamg_csr** A_out, mlamg_halo** halo_out);

#ifdef __cplusplus
}
#endif
#endif /* MLAMG_H_ */
