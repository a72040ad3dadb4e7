"""The reference's AMG loss of a prolongator and its gradient with respect to P, on the device.

Reference: ns/model/loss.py:32-96 (amg_loss). It scores an interpolation operator P by running
tot_num_loop + 1 two-level cycles on a block of k test vectors with a zero right-hand side
(pre-relaxation, coarse-grid correction, post-relaxation, mean removal: loss.py:70-89), records
||x_j||_2 of every column after each cycle (loss.py:90) and turns the last three rows of that
history into per-column convergence factors convs = (errs[-1] / errs[-3]) ** (1/2) and the
softmax-weighted loss softmax(convs) @ convs (loss.py:92-94).

Here the cycles run through the block V-cycle of the library (Hierarchy.cycle_multi,
mlamg_hier_vcycle_mv): every operator is streamed once for all k columns. The coarse system is
solved by the dense inverse up to Hierarchy.TWO_LEVEL_DENSE_MAX rows and by the block PCG
(mlamg_pcg_solve_mv, to a relative residual of 1e-12) above, where the reference factorises
A_H with a sparse direct solver at any size (loss.py:79).

Differences from the reference, all stated:
  * fp64 throughout. The reference holds x, A and P in fp32 and only solves the coarse system in
    fp64 (loss.py:54,59,79). torch_sparse / torch_sparse_solve, which the reference needs, are
    not available to this project's tests, so its fp32 numbers are parity-unpinned: the tests pin
    the history bit for bit to the library's single-vector cycle and to an fp64 numpy/scipy
    restatement of loss.py:48-96 within the project's SuperLU-versus-dense bounds.
  * differentiable with respect to P's stored values only (amg_loss_and_grad, and the torch
    autograd surface amg_loss_values): the adjoint two-level cycle below, not torch autograd
    through the kernels. A and the test vectors are constants; asking for their gradients raises
    NotImplementedError. With a PCG coarse solve the adjoint treats the solve as exact (implicit
    differentiation: the PCG iteration itself is not differentiated), so the gradient carries an
    error of order rtol * cond(A_H) = 1e-12 cond(A_H) relative to the dense-coarse gradient. A
    GMRES coarse solve (an A_H that is not symmetric, beyond the dense solver's size) is not
    differentiated: NotImplementedError.
  * neumann_solve_fix=True (the Lagrange-row coarse system, loss.py:11-30,66-67,76-82) is not
    implemented and raises NotImplementedError, forward and backward.

The gradient. One forward cycle is, with A fixed, D = (2/3) / diag A and
A_H = P^T A P:  x <- x - D A x (nu1 times);  e = -A_H^-1 P^T A x;  x2 = x + P e;
x <- x - D A x (nu2 times);  x4 = x - mean(x);  errs[c] = ||x4||_2 per column. The backward pass
runs the cycles last to first on the cotangent g of x (n x k, starting at 0), with dP on P's
pattern:
  1. g += x4 diag(ebar[c] / errs[c])         (ebar is nonzero for the last and third-last cycle)
  2. g <- g - colmean(g)
  3. nu2 times: g <- g - A^T (D g)
  4. lam = -A_H^-T (P^T g)                   (dense inverse, or PCG: A_H passed the symmetry
                                              test, so the forward's solver serves A_H^T too)
  5. g <- g + A^T (P lam)
  6. dP += sample_P[g e^T + (A x2) lam^T]    (two mlamg_sddmm launches on P's handle)
  7. nu1 times: g <- g - A^T (D g)
No n_c x n_c cotangent of A_H is formed: the Galerkin, restriction and prolongation terms
collapse into the two rank-k sampled products of step 6.

A batch of problems: AmgLossBatch evaluates nb independent (A_i, P_i) as one
problem on their block-diagonal stack, the same forward and backward with a segmented mean
removal and norm and a block-diagonal coarse inverse; problem i's history, loss and gradient are
bitwise the single call's.
"""
from __future__ import annotations

import numpy as np

__all__ = ["amg_loss", "amg_loss_and_grad", "amg_loss_values", "loss_from_errs",
           "AmgLossBatch", "amg_loss_batch", "amg_loss_and_grad_batch", "stack_problems",
           "BlockDense"]

_NEUMANN_MSG = ("neumann_solve_fix=True (the Lagrange-row coarse system of "
                "ns/model/loss.py:11-30) is not implemented")


def loss_from_errs(errs, n_err=3):
    """(loss, convs) of an error history errs[(cycles, k)] (ns/model/loss.py:92-94):
    convs = (errs[-1] / errs[-n_err]) ** (1 / (n_err - 1)) per column and
    loss = softmax(convs) @ convs. Pure host arithmetic in fp64."""
    errs = np.asarray(errs, dtype=np.float64)
    if errs.ndim != 2 or errs.shape[0] < n_err:
        raise ValueError(f"errs must be (cycles >= {n_err}, k), got shape {errs.shape}")
    convs = (errs[-1] / errs[-n_err]) ** (1.0 / (n_err - 1))
    w = np.exp(convs - convs.max())
    w = w / w.sum()
    return float(w @ convs), convs


def _as_operator(M):
    """scipy sparse / DeviceCSR / torch sparse -> something Hierarchy.two_level uploads."""
    import scipy.sparse as sp
    import torch
    from .sparse import DeviceCSR, to_scipy
    if isinstance(M, DeviceCSR) or sp.issparse(M):
        return M
    if isinstance(M, torch.Tensor):
        if M.layout == torch.sparse_coo:
            return to_scipy(M).astype(np.float64)
        if M.layout == torch.sparse_csr:
            return sp.csr_matrix((M.values().cpu().numpy().astype(np.float64),
                                  M.col_indices().cpu().numpy(),
                                  M.crow_indices().cpu().numpy()), shape=tuple(M.shape))
        raise TypeError("a torch operator must be sparse (COO or CSR)")
    raise TypeError(f"unsupported operator type {type(M).__name__}")


def amg_loss(P, A, test_vecs, tot_num_loop=5, no_prerelax=1, no_postrelax=1,
             neumann_solve_fix=False, return_factors=False):
    """ns/model/loss.py:32-96 in fp64 on the device (see the module docstring for the
    differences: the reference runs fp32 with an fp64 coarse solve, and that fp32 path is
    parity-unpinned here).

    P, A       scipy sparse, DeviceCSR or torch sparse: N_F x N_C prolongator, N_F x N_F system
    test_vecs  int k: np.random.seed(0) normal (N_F, k) vectors, column-normalised
               (loss.py:58-60); or an (N_F, k) array / tensor used as given. k <= 64.
    Any coarse size: the dense inverse, or the block PCG above Hierarchy.TWO_LEVEL_DENSE_MAX
    rows (a breakdown raises CoarseSolveError); a GMRES coarse solve raises MlamgError
    (EUNSUPPORTED).
    Returns the loss (float); with return_factors=True, (loss, convs, errs) with errs the
    (tot_num_loop + 1, k) history of ||x_j||_2 after each cycle."""
    if neumann_solve_fix:
        raise NotImplementedError("amg_loss: " + _NEUMANN_MSG)
    import torch
    from .hierarchy import Hierarchy
    from .sparse import to_device_vec
    A = _as_operator(A)
    P = _as_operator(P)
    n = A.shape[0]
    if isinstance(test_vecs, (int, np.integer)):
        np.random.seed(0)
        x = np.random.normal(0, 1, (n, int(test_vecs)))
        x = x / np.linalg.norm(x, 2, axis=0)
    else:
        x = test_vecs
    X = to_device_vec(x)
    if isinstance(x, torch.Tensor) and X.data_ptr() == x.data_ptr():
        X = X.clone()  # the cycle runs in place; the caller's vectors stay as they are
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"test_vecs must be ({n}, k), got {tuple(X.shape)}")
    H = Hierarchy.two_level(A, P, omega=2.0 / 3.0, nu_pre=int(no_prerelax),
                            nu_post=int(no_postrelax))
    errs = H.cycle_multi(None, X, int(tot_num_loop) + 1, norm="x", remove_mean=True)
    loss, convs = loss_from_errs(errs)
    return (loss, convs, errs) if return_factors else loss


# ---------------------------------------------------------------------- gradient w.r.t. P
def _refuse_grad_of(A, test_vecs, who):
    """Only P's values are differentiable: a silent zero gradient is worse than an error."""
    import torch
    if isinstance(test_vecs, torch.Tensor) and test_vecs.requires_grad:
        raise NotImplementedError(f"{who}: test_vecs requires grad, but the gradient with "
                                  "respect to the test vectors is not implemented (detach it)")
    if isinstance(A, torch.Tensor) and A.requires_grad:
        raise NotImplementedError(f"{who}: A requires grad, but the gradient with respect to "
                                  "A is not implemented (detach it)")


def _check_canonical(indptr, indices, shape, nnz):
    """ValueError unless (indptr, indices) is a canonical CSR pattern of `shape` with nnz
    entries: column indices strictly ascending within every row."""
    indptr = np.asarray(indptr)
    indices = np.asarray(indices)
    if indptr.ndim != 1 or indptr.size != shape[0] + 1 or indices.ndim != 1:
        raise ValueError(f"P: indptr must have {shape[0] + 1} entries")
    if indptr[0] != 0 or indptr[-1] != nnz or indices.size != nnz \
            or np.any(np.diff(indptr) < 0):
        raise ValueError("P: indptr, indices and values do not describe one CSR matrix")
    if nnz and (indices.min() < 0 or indices.max() >= shape[1]):
        raise ValueError("P: a column index is out of range")
    if nnz > 1:
        rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
        if np.any((rows[1:] == rows[:-1]) & (indices[1:] <= indices[:-1])):
            raise ValueError("P is not in canonical CSR form (sorted column indices, no "
                             "duplicates): the gradient is returned in P's stored order")


def _canonical_P(P):
    """P as something Hierarchy.two_level uploads with its stored order unchanged; ValueError
    for a P that is not canonical (the gradient's order would not be the caller's)."""
    import scipy.sparse as sp
    import torch
    from .sparse import DeviceCSR
    if isinstance(P, torch.Tensor) and P.layout == torch.sparse_coo and not P.is_coalesced():
        raise ValueError("P is not in canonical form: a torch COO prolongator must be coalesced")
    if isinstance(P, DeviceCSR):
        S = P.to_scipy()
    else:
        S = _as_operator(P)
        S = S if sp.isspmatrix_csr(S) else S.tocsr()
        P = S
    _check_canonical(S.indptr, S.indices, S.shape, S.nnz)
    return P


# The recorded forward, the host cotangents and the adjoint sweep, shared by the single call
# (_loss_and_grad_device) and the batch (AmgLossBatch). What differs between the two comes in as
# callables: coarse_solve / solve_T (rhs, out), remove_mean (V) and norm (V, out).
def _recorded_forward(Ad, Pd, Rd, dinv, X, T, nu1, nu2, coarse_solve, remove_mean, norm,
                      errs_shape, record=True):
    """T + 1 two-level cycles on X (n x k, in place) with the block cycle's own steps
    (csrc/hier_mv.hip mlamg_hier_vcycle_mv); norm writes each cycle's row of errs_d
    ((T + 1,) + errs_shape). record: keep x after the coarse correction (X2) and the coarse
    correction (E) of every cycle and x after the mean removal (X4) of the two cycles the loss
    reads, for the adjoint sweep. Returns the record and the work blocks."""
    import torch
    from ._lib import call, ptr, stream_ptr
    n, k = X.shape
    nc = Pd.shape[1]
    dev = X.device
    s = stream_ptr()

    def block(rows, *lead):
        return torch.empty(lead + (rows, k), dtype=torch.float64, device=dev)

    ncyc = T + 1
    X2 = block(n, ncyc) if record else None   # x after the coarse correction, per cycle
    E = block(nc, ncyc if record else 1)      # the coarse correction e, per cycle
    X4 = {}                # x after the mean removal, for the two cycles the loss reads
    tmp, r, bc = block(n), block(n), block(nc)
    errs_d = torch.empty((ncyc,) + tuple(errs_shape), dtype=torch.float64, device=dev)
    for c in range(ncyc):
        e = E[c] if record else E[0]
        if nu1:
            call("mlamg_jacobi_mv", Ad.handle, ptr(dinv), None, 0, ptr(X), k, ptr(tmp), k, k,
                 nu1, s)
        call("mlamg_residual_mv", Ad.handle, None, 0, ptr(X), k, ptr(r), k, k, None, s)
        call("mlamg_restrict_mv", Rd.handle, ptr(r), k, ptr(bc), k, k, s)
        coarse_solve(bc, e)
        call("mlamg_prolong_add_mv", Pd.handle, ptr(e), k, ptr(X), k, k, s)
        if record:
            X2[c].copy_(X)
        if nu2:
            call("mlamg_jacobi_mv", Ad.handle, ptr(dinv), None, 0, ptr(X), k, ptr(tmp), k, k,
                 nu2, s)
        remove_mean(X)
        norm(X, errs_d[c])
        if record and c in (T, T - 2):
            X4[c] = X.clone()
    return {"X2": X2, "E": E, "X4": X4, "tmp": tmp, "r": r, "bc": bc, "errs_d": errs_d}


def _history_cotangents(errs, T):
    """(loss, convs, {cycle: d loss / d errs[cycle] / errs[cycle]}) of one problem's error
    history errs ((T + 1, k)): host arithmetic on k numbers. The two entries scale x4 of the
    last and the third-last cycle in step 1 of the backward pass."""
    loss, convs = loss_from_errs(errs)
    w = np.exp(convs - convs.max())
    w = w / w.sum()
    dconv = w * (1.0 + convs - loss)
    scale = {T: dconv * convs / (2.0 * errs[T]) / errs[T],
             T - 2: -dconv * convs / (2.0 * errs[T - 2]) / errs[T - 2]}
    return loss, convs, scale


def _adjoint_jacobi_operator(Ad, dinv):
    """(D A)^T on the device: one adjoint Jacobi sweep is g - M g."""
    import ctypes

    from ._lib import call, ptr, stream_ptr
    from .sparse import DeviceCSR
    h = ctypes.c_void_p()
    call("mlamg_csr_scale_rows", Ad.handle, ptr(dinv), 0, ctypes.byref(h), stream_ptr())
    return DeviceCSR(h).transpose()


def _adjoint_sweep(Ad, AT, M, Pd, Rd, X, rec, scale, T, nu1, nu2, solve_T, remove_mean):
    """The backward pass of the module docstring over the recorded cycles, last to first; dP
    (cuda, length nnz(P)) in P's stored order. scale[c] multiplies x4 of cycle c: a (k,) tensor,
    or (n, k) with one row of factors per row of x. X and the forward's work blocks are
    reused."""
    import torch
    from ._lib import call, ptr, stream_ptr
    n, k = X.shape
    dev = X.device
    s = stream_ptr()
    X2, E, X4 = rec["X2"], rec["E"], rec["X4"]

    def adjoint_jacobi(g, g2, nu):
        for _ in range(nu):
            g2.copy_(g)
            M.matmat(g, out=g2, alpha=-1.0, beta=1.0)
            g, g2 = g2, g
        return g, g2

    g = torch.zeros((n, k), dtype=torch.float64, device=dev)
    g2, q, ax2 = rec["tmp"], rec["r"], X  # the forward's work blocks, free now
    t, lam = rec["bc"], torch.empty_like(rec["bc"])
    dP = torch.zeros(Pd.nnz, dtype=torch.float64, device=dev)
    for c in range(T, -1, -1):
        if c in scale:
            g.addcmul_(X4[c], scale[c])
        remove_mean(g)
        g, g2 = adjoint_jacobi(g, g2, nu2)
        call("mlamg_restrict_mv", Rd.handle, ptr(g), k, ptr(t), k, k, s)
        solve_T(t, lam)
        lam.neg_()
        Pd.matmat(lam, out=q)
        AT.matmat(q, out=g, alpha=1.0, beta=1.0)
        Ad.matmat(X2[c], out=ax2)
        Pd.sddmm(g, E[c], alpha=1.0, beta=1.0, out=dP)
        Pd.sddmm(ax2, lam, alpha=1.0, beta=1.0, out=dP)
        if c:  # the cotangent of the starting vectors is not asked for
            g, g2 = adjoint_jacobi(g, g2, nu1)
    return dP


def _loss_and_grad_device(P, A, test_vecs, tot_num_loop, no_prerelax, no_postrelax):
    """(loss, dP as a cuda tensor in the stored order of the canonical P, convs, errs)."""
    import torch
    from ._lib import call, ptr, stream_ptr
    from .hierarchy import Hierarchy, csr_symmetric
    from .sparse import mv_block, to_device_vec
    T, nu1, nu2 = int(tot_num_loop), int(no_prerelax), int(no_postrelax)
    if T < 2:
        raise ValueError(f"tot_num_loop must be >= 2 (the loss reads errs[-3]), got {T}")
    if nu1 < 0 or nu2 < 0:
        raise ValueError("no_prerelax and no_postrelax must be >= 0")
    A = _as_operator(A)
    n = A.shape[0]
    if isinstance(test_vecs, (int, np.integer)):
        np.random.seed(0)
        x = np.random.normal(0, 1, (n, int(test_vecs)))
        x = x / np.linalg.norm(x, 2, axis=0)
    else:
        x = test_vecs.detach() if isinstance(test_vecs, torch.Tensor) else test_vecs
    X = to_device_vec(x)
    if isinstance(x, torch.Tensor) and X.data_ptr() == x.data_ptr():
        X = X.clone()
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"test_vecs must be ({n}, k), got {tuple(X.shape)}")
    k, _ = mv_block(X, n, "test_vecs")
    H = Hierarchy.two_level(A, P, omega=2.0 / 3.0, nu_pre=nu1, nu_post=nu2)
    if H.dense is None and H.pcg is None:
        raise NotImplementedError(
            f"amg_loss_and_grad: the coarse operator of {H.Ac.shape[0]} rows is not symmetric "
            "and beyond the dense coarse solve, so its coarse solve is GMRES, which is not "
            "differentiated (dense and PCG coarse solves are)")
    L = H.levels[0]
    Ad, Pd, Rd, dinv = L.A, L.P, L.R, L.dinv
    dev = X.device
    s = stream_ptr()

    def coarse_solve(rhs, out):
        # the forward's solver; PCG was chosen because A_H is symmetric, so it is A_H^-T too
        if H.pcg is not None:
            call("mlamg_pcg_solve_mv", H.pcg, ptr(rhs), k, ptr(out), k, k, s)
        else:
            call("mlamg_dense_solve_mv", H.dense, ptr(rhs), k, ptr(out), k, k, s)

    def remove_mean(V):
        call("mlamg_remove_mean_mv", ptr(V), k, n, k, s)

    def norm(V, out):
        call("mlamg_norm2_mv", ptr(V), k, n, k, ptr(out), s)

    rec = _recorded_forward(Ad, Pd, Rd, dinv, X, T, nu1, nu2, coarse_solve, remove_mean, norm,
                            (k,))
    errs = rec["errs_d"].cpu().numpy()
    H.check_coarse()  # a PCG breakdown in the forward: CoarseSolveError
    loss, convs, scale = _history_cotangents(errs, T)
    scale = {c: torch.as_tensor(v, dtype=torch.float64).to(dev) for c, v in scale.items()}

    # ---- adjoint operators, built once
    M = _adjoint_jacobi_operator(Ad, dinv)
    HT = None
    if csr_symmetric(Ad, 0.0):
        AT, solve_T = Ad, coarse_solve
    else:
        AT = Ad.transpose()
        if H.pcg is not None:  # A_H symmetric to rounding though A is not exactly symmetric
            solve_T = coarse_solve
        else:
            HT = Hierarchy.two_level(AT, Pd, omega=2.0 / 3.0, coarse="dense")  # A_c = A_H^T

            def solve_T(rhs, out):
                call("mlamg_dense_solve_mv", HT.dense, ptr(rhs), k, ptr(out), k, k, s)

    dP = _adjoint_sweep(Ad, AT, M, Pd, Rd, X, rec, scale, T, nu1, nu2, solve_T, remove_mean)
    torch.cuda.current_stream().synchronize()  # HT / M are released on return
    H.check_coarse()  # a PCG breakdown in the backward solves
    return loss, dP, convs, errs


def amg_loss_and_grad(P, A, test_vecs, tot_num_loop=5, no_prerelax=1, no_postrelax=1,
                      neumann_solve_fix=False, return_factors=False):
    """amg_loss and its gradient with respect to P's stored values: (loss, grad), or with
    return_factors=True (loss, grad, convs, errs).

    P, A, test_vecs and the cycle parameters are amg_loss's. grad is a numpy fp64 array of
    length nnz(P) in the order of P's canonical CSR (sorted column indices, no duplicates; for
    a coalesced torch COO P the order of P.values()). A P that is not canonical raises
    ValueError. The recorded forward runs the block cycle's own primitives step by step, so
    errs (and the loss) are bitwise amg_loss's. The backward pass is the adjoint cycle of the
    module docstring: SpMM launches on A^T, (D A)^T, P and P^T, the coarse solve on A_H^T and
    two mlamg_sddmm launches per cycle. The coarse solve is the forward's: the dense inverse
    (its handle when A is exactly symmetric, else a second two-level setup on A^T), or above
    Hierarchy.TWO_LEVEL_DENSE_MAX rows the block PCG (mlamg_pcg_solve_mv), forward and backward
    on the same solver, since PCG is only chosen for an A_H that passed the symmetry test. The
    adjoint treats the PCG solve as exact (implicit differentiation), so against the
    dense-coarse gradient the result differs by the order of rtol * cond(A_H) (rtol = 1e-12;
    DESIGN.md §20 has the measured figures). A PCG breakdown in either pass raises
    CoarseSolveError.

    Memory held between the forward and the backward pass: x2 and e of every cycle and x4 of
    two, (tot_num_loop + 1) (n + n_c) k + 2 n k doubles, plus five n x k and three n_c x k
    work blocks.

    Refused: neumann_solve_fix=True (NotImplementedError), a GMRES coarse solve (a coarse
    operator that is not symmetric and beyond the dense solver's size: NotImplementedError),
    k > 64 and tot_num_loop < 2 (ValueError), test_vecs or A requiring grad
    (NotImplementedError)."""
    if neumann_solve_fix:
        raise NotImplementedError("amg_loss_and_grad: " + _NEUMANN_MSG)
    _refuse_grad_of(A, test_vecs, "amg_loss_and_grad")
    P = _canonical_P(P)
    loss, dP, convs, errs = _loss_and_grad_device(P, A, test_vecs, tot_num_loop, no_prerelax,
                                                  no_postrelax)
    grad = dP.cpu().numpy()
    return (loss, grad, convs, errs) if return_factors else (loss, grad)


_AmgLossFn = None


def _autograd_fn():
    """The torch.autograd.Function of amg_loss_values (built on first use: torch is imported
    lazily in this module)."""
    global _AmgLossFn
    if _AmgLossFn is not None:
        return _AmgLossFn
    import torch
    from torch.autograd.function import once_differentiable

    class AmgLossFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values, P, A, test_vecs, tot_num_loop, no_prerelax, no_postrelax):
            loss, dP, _, _ = _loss_and_grad_device(P, A, test_vecs, tot_num_loop, no_prerelax,
                                                   no_postrelax)
            ctx.save_for_backward(dP.to(values.device))
            return torch.tensor(loss, dtype=torch.float64, device=values.device)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            (dP,) = ctx.saved_tensors
            return grad_output * dP, None, None, None, None, None, None

    _AmgLossFn = AmgLossFn
    return _AmgLossFn


def amg_loss_values(values, indptr, indices, shape, A, test_vecs, tot_num_loop=5,
                    no_prerelax=1, no_postrelax=1, neumann_solve_fix=False):
    """amg_loss of the prolongator csr(values, indices, indptr) of `shape`, as a 0-dim fp64
    tensor on values.device that torch autograd can differentiate with respect to `values`.

    values   fp64 torch tensor of P's stored entries in canonical CSR order (cuda, or cpu and
             uploaded); indptr / indices: the pattern (numpy arrays or torch tensors).
    If values.requires_grad the result carries the grad_fn of a torch.autograd.Function whose
    backward returns grad_output * d loss / d values (amg_loss_and_grad's array, computed
    with the forward) and None for everything else; otherwise it is amg_loss's float. Only P's
    values are differentiable: a test_vecs tensor or a torch A that requires grad raises
    NotImplementedError naming the argument. Dense and PCG coarse solves as in
    amg_loss_and_grad; a GMRES coarse solve raises NotImplementedError. Not twice differentiable
    (the backward is once_differentiable: a second derivative raises)."""
    import torch
    from .sparse import DeviceCSR, _device
    if neumann_solve_fix:
        raise NotImplementedError("amg_loss_values: " + _NEUMANN_MSG)
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float64 \
            or values.ndim != 1:
        raise TypeError("values must be a 1-D float64 torch tensor")
    _refuse_grad_of(A, test_vecs, "amg_loss_values")
    shape = (int(shape[0]), int(shape[1]))

    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    ip, ix = host(indptr), host(indices)
    _check_canonical(ip, ix, shape, values.numel())
    dev = _device()
    P = DeviceCSR.from_torch(torch.as_tensor(ip.astype(np.int32)).to(dev),
                             torch.as_tensor(ix.astype(np.int32)).to(dev),
                             values.detach().to(dev).contiguous(), shape)
    if values.requires_grad and torch.is_grad_enabled():
        return _autograd_fn().apply(values, P, A, test_vecs, int(tot_num_loop),
                                    int(no_prerelax), int(no_postrelax))
    loss = amg_loss(P, A, test_vecs, tot_num_loop, no_prerelax, no_postrelax)
    return torch.tensor(loss, dtype=torch.float64, device=values.device)


# ---------------------------------------------------------------------- a batch of problems
# DESIGN.md §24. nb independent problems (A_i, P_i) are evaluated as one problem on the
# block-diagonal stack: every row-wise kernel of the single path works per row or per stored entry,
# so on the stack it computes each problem's rows with the bits of the single call; the three
# things that couple the rows of a stack (per-column mean, per-column norm, the coarse inverse)
# have segmented / block-diagonal device code (csrc/seg_mv.hip, csrc/blockdense.hip).
BATCH_MAX_PROBLEMS = 65535  # a grid dimension of the segmented kernels


def batch_coarse_max_rows():
    """Coarse blocks of this many rows or more are refused by the batch: mlamg_dense_create keeps
    the Cholesky factor there (method 2), which the block-diagonal inverse does not build
    (dense.hip dense_tri_min: 2048, or MLAMG_DENSE_TRI_MIN)."""
    import os
    e = os.environ.get("MLAMG_DENSE_TRI_MIN")
    return int(e) if e else 2048


def _check_stack_int32(n_rows, nnz_A, nnz_P):
    """ValueError when the stack does not fit the int32 indices of the device CSR handle."""
    lim = 2**31 - 1
    for what, v in (("row count", n_rows), ("nnz of A", nnz_A), ("nnz of P", nnz_P)):
        if v >= lim:
            raise ValueError(f"the stacked {what} ({v}) exceeds the int32 index range of the "
                             "device CSR handle: split the batch")


def _stack_csr(mats, col_offsets, n_cols):
    """The block-diagonal stack of CSR matrices with every row's stored order kept (block i's
    columns shifted by col_offsets[i])."""
    import scipy.sparse as sp
    nnz_off = np.concatenate([[0], np.cumsum([m.nnz for m in mats])]).astype(np.int64)
    indptr = np.concatenate([[0]] + [m.indptr[1:].astype(np.int64) + nnz_off[i]
                                     for i, m in enumerate(mats)])
    indices = np.concatenate([m.indices.astype(np.int64) + col_offsets[i]
                              for i, m in enumerate(mats)])
    data = np.concatenate([np.asarray(m.data, dtype=np.float64) for m in mats])
    S = sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)),
                      shape=(len(indptr) - 1, int(n_cols)))
    return S, nnz_off


def stack_problems(As, Ps):
    """The block-diagonal stack of nb problems (scipy CSR A_i: n_i x n_i, P_i: n_i x nc_i), pure
    numpy / scipy. Returns a namespace with
      A, P                      the stacked CSR matrices (stored order of every row kept: for
                                canonical inputs scipy.sparse.block_diag(...).tocsr())
      row_offsets, coarse_offsets, nnz_offsets
                                int64 arrays of nb + 1 entries: problem i owns the rows
                                [row_offsets[i], row_offsets[i + 1]) of A and P, the columns
                                [coarse_offsets[i], ...) of P and the stored entries
                                [nnz_offsets[i], ...) of P
      row_seg, entry_seg        the problem of every row / of every stored entry of P (int64)"""
    import types
    nb = len(As)
    if nb < 1 or len(Ps) != nb:
        raise ValueError(f"a batch needs as many prolongators as operators, at least one "
                         f"(got {nb} and {len(Ps)})")
    for i, (A, P) in enumerate(zip(As, Ps)):
        if A.shape[0] != A.shape[1]:
            raise ValueError(f"problem {i}: A must be square, got {A.shape}")
        if P.shape[0] != A.shape[0]:
            raise ValueError(f"problem {i}: P has {P.shape[0]} rows, A has {A.shape[0]}")
    row_off = np.concatenate([[0], np.cumsum([A.shape[0] for A in As])]).astype(np.int64)
    crs_off = np.concatenate([[0], np.cumsum([P.shape[1] for P in Ps])]).astype(np.int64)
    _check_stack_int32(int(row_off[-1]), sum(A.nnz for A in As), sum(P.nnz for P in Ps))
    A, _ = _stack_csr(As, row_off, row_off[-1])
    P, nnz_off = _stack_csr(Ps, crs_off, crs_off[-1])
    seg = np.arange(nb, dtype=np.int64)
    return types.SimpleNamespace(
        A=A, P=P, row_offsets=row_off, coarse_offsets=crs_off, nnz_offsets=nnz_off,
        row_seg=np.repeat(seg, np.diff(row_off)), entry_seg=np.repeat(seg, np.diff(nnz_off)))


def _batch_host_setup(As, Ps, test_vecs):
    """Everything of AmgLossBatch's constructor that needs no device: the refusals (each names
    the problem), the stack, the test vectors and the exact-symmetry test per problem."""
    import scipy.sparse as sp
    import torch
    from .sparse import MV_MAX, DeviceCSR, canonical_rows
    As, Ps = list(As), list(Ps)
    nb = len(As)
    if nb < 1 or len(Ps) != nb:
        raise ValueError(f"a batch needs as many prolongators as operators, at least one "
                         f"(got {nb} and {len(Ps)})")
    if nb > BATCH_MAX_PROBLEMS:
        raise ValueError(f"a batch takes at most {BATCH_MAX_PROBLEMS} problems, got {nb}")
    given = not isinstance(test_vecs, (int, np.integer))
    if given:
        test_vecs = list(test_vecs)
        if len(test_vecs) != nb:
            raise ValueError(f"test_vecs has {len(test_vecs)} blocks for {nb} problems")
        k = None
    else:
        k = int(test_vecs)
        if not 1 <= k <= MV_MAX:
            raise ValueError(f"test_vecs = {k} columns; the block path takes 1 to {MV_MAX}")
    thr = batch_coarse_max_rows()
    A_s, P_s, X_s = [], [], []
    for i in range(nb):
        _refuse_grad_of(As[i], test_vecs[i] if given else None, f"AmgLossBatch (problem {i})")
        try:
            P = _canonical_P(Ps[i])
        except ValueError as e:
            raise ValueError(f"problem {i}: {e}") from None
        P = P.to_scipy() if isinstance(P, DeviceCSR) else P
        A = _as_operator(As[i])
        A = A.to_scipy() if isinstance(A, DeviceCSR) else A
        A = canonical_rows(sp.csr_matrix(A, dtype=np.float64))
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError(f"problem {i}: A must be square, got {A.shape}")
        if P.shape[0] != n:
            raise ValueError(f"problem {i}: P has {P.shape[0]} rows, A has {n}")
        if P.shape[1] >= thr:
            raise ValueError(
                f"problem {i}: its coarse block of {P.shape[1]} rows is at or above the factored "
                f"dense solve's threshold ({thr} rows); the batch is for small coarse problems: "
                "use the single call (amg_loss_and_grad) for this one")
        if given:
            x = test_vecs[i]
            x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            x = np.ascontiguousarray(x, dtype=np.float64)
            if x.ndim != 2 or x.shape[0] != n:
                raise ValueError(f"problem {i}: test_vecs must be ({n}, k), got {x.shape}")
            if not 1 <= x.shape[1] <= MV_MAX:
                raise ValueError(f"problem {i}: test_vecs has {x.shape[1]} columns; the block "
                                 f"path takes 1 to {MV_MAX}")
            if k is None:
                k = x.shape[1]
            if x.shape[1] != k:
                raise ValueError(f"problem {i}: test_vecs has {x.shape[1]} columns, problem 0 "
                                 f"has {k}: k is the same for all problems")
            X_s.append(x)
        A_s.append(A)
        P_s.append(sp.csr_matrix(P, dtype=np.float64))
    st = stack_problems(A_s, P_s)
    if not given:  # what amg_loss(P_i, A_i, k) generates, per problem
        for A in A_s:
            np.random.seed(0)
            x = np.random.normal(0, 1, (A.shape[0], k))
            X_s.append(x / np.linalg.norm(x, 2, axis=0))
    st.X = np.concatenate(X_s, axis=0)
    st.k = k
    # exactly symmetric problems keep A itself as A^T (the single call's csr_symmetric(A, 0)
    # branch); the others get the transpose in sorted order, as mlamg_transpose stores it
    st.sym = []
    for A in A_s:
        D = (A - A.T).tocsr()
        st.sym.append(bool(D.nnz == 0 or np.all(D.data == 0.0)))
    st.AT = None
    if not all(st.sym):
        ATs = []
        for A, sym in zip(A_s, st.sym):
            if sym:
                ATs.append(A)
            else:
                At = sp.csr_matrix(A.T)
                At.sort_indices()
                ATs.append(At)
        st.AT, _ = _stack_csr(ATs, st.row_offsets, st.row_offsets[-1])
    return st


class BlockDense:
    """The inverses of the diagonal blocks of a device CSR (mlamg_blockdense: block b bitwise
    mlamg_dense_create on that block alone). offsets: nb + 1 host row offsets."""

    def __init__(self, Ac, offsets):
        import ctypes

        from ._lib import call, stream_ptr
        self.handle = None
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.nb = self.offsets.size - 1
        h = ctypes.c_void_p()
        call("mlamg_blockdense_create", Ac.handle,
             self.offsets.ctypes.data_as(ctypes.c_void_p), self.nb, ctypes.byref(h), stream_ptr())
        self.handle = h

    def methods(self):
        """mlamg_dense_info's method per block (0 Gauss-Jordan, 1 inverse Cholesky factor)."""
        import ctypes

        from ._lib import call
        m = (ctypes.c_int * self.nb)()
        call("mlamg_blockdense_info", self.handle, None, None, m)
        return list(m)

    def solve(self, B, out):
        """out_b = inv_b B_b on stacked (n_c, k) cuda fp64 blocks."""
        from ._lib import call, ptr, stream_ptr
        from .sparse import mv_block
        n = int(self.offsets[-1])
        k, ldb = mv_block(B, n, "B")
        ko, ldx = mv_block(out, n, "out")
        if ko != k:
            raise ValueError(f"out has {ko} columns, B has {k}")
        call("mlamg_blockdense_solve_mv", self.handle, ptr(B), ldb, ptr(out), ldx, k,
             stream_ptr())
        return out

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                from ._lib import lib
                lib.mlamg_blockdense_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self.handle = None


class AmgLossBatch:
    """amg_loss and its gradient for nb independent problems (A_i, P_i) as one problem on the
    block-diagonal stack: every operator is streamed once per step for the whole batch and the
    launch count does not depend on nb. PROBLEM i's ERROR HISTORY, LOSS AND GRADIENT ARE BITWISE
    WHAT amg_loss_and_grad(P_i, A_i, X_i, ...) RETURNS.

    As, Ps     lists of nb operators / canonical prolongators (what amg_loss_and_grad takes)
    test_vecs  int k: problem i gets np.random.seed(0) normal (n_i, k) columns, normalised
               (what amg_loss(P_i, A_i, k) generates); or a list of (n_i, k) arrays / tensors.
               k is the same for all problems, at most 64.
    The constructor does once what does not depend on P's values: it stacks and uploads A,
    builds dinv, (D A)^T and, when a problem is not exactly symmetric, A^T, and records P's
    stacked pattern, the row / coarse / nnz offsets (attributes row_offsets, coarse_offsets,
    nnz_offsets) and the problem of every row and entry. Every step uploads the stacked values,
    forms R = P^T and the Galerkin product, inverts the coarse blocks (BlockDense; a second
    inverse on galerkin(R, A^T, P) when the stack is not symmetric, as the single call's second
    two-level setup) and runs the recorded forward and the adjoint sweep of the single path with
    the segmented mean removal and norm.

    values (every method): the stored values of all P_i, concatenated in problem order (numpy
    array or torch tensor of nnz_offsets[-1] entries), or a list of per-problem arrays.

    Refused on the host, before any device work, naming the problem where one applies:
    neumann_solve_fix=True, a P that is not canonical, mismatched shapes, k > 64, test_vecs or
    A requiring grad, a coarse block at or above batch_coarse_max_rows() rows (use the single
    call), a stack beyond int32; tot_num_loop < 2 when a gradient is asked for."""

    def __init__(self, As, Ps, test_vecs, tot_num_loop=5, no_prerelax=1, no_postrelax=1,
                 neumann_solve_fix=False):
        if neumann_solve_fix:
            raise NotImplementedError("AmgLossBatch: " + _NEUMANN_MSG)
        self.T, self.nu1, self.nu2 = int(tot_num_loop), int(no_prerelax), int(no_postrelax)
        if self.T < 0:
            raise ValueError("tot_num_loop must be >= 0")
        if self.nu1 < 0 or self.nu2 < 0:
            raise ValueError("no_prerelax and no_postrelax must be >= 0")
        st = _batch_host_setup(As, Ps, test_vecs)
        import torch
        from .sparse import DeviceCSR, _device
        dev = _device()
        self.nb = len(st.sym)
        self.k = st.k
        self.row_offsets, self.coarse_offsets = st.row_offsets, st.coarse_offsets
        self.nnz_offsets = st.nnz_offsets
        self.n, self.nc, self.nnz = (int(st.row_offsets[-1]), int(st.coarse_offsets[-1]),
                                     int(st.nnz_offsets[-1]))
        self.max_len = int(np.diff(st.row_offsets).max())
        self.symmetric = all(st.sym)
        self.profile = False      # True: time the phases of a step (synchronising) into .phases
        self.phases = {}
        self.Ad = DeviceCSR.from_scipy(st.A, check=False)
        self.dinv = self.Ad.diag_inv(2.0 / 3.0)
        self.M = _adjoint_jacobi_operator(self.Ad, self.dinv)
        self.AT = self.Ad if self.symmetric else DeviceCSR.from_scipy(st.AT, check=False)
        self._p_crow = torch.as_tensor(st.P.indptr.astype(np.int32)).to(dev)
        self._p_col = torch.as_tensor(st.P.indices.astype(np.int32)).to(dev)
        self._row_off_d = torch.as_tensor(st.row_offsets).to(dev)
        self._row_seg_d = torch.as_tensor(st.row_seg).to(dev)
        self._entry_seg = torch.as_tensor(st.entry_seg)
        self._entry_seg_d = {}
        self.X0 = torch.as_tensor(st.X).to(dev)

    # ------------------------------------------------------------------ values
    def _values(self, values):
        import torch
        from .sparse import _device
        if isinstance(values, (list, tuple)):
            if len(values) != self.nb:
                raise ValueError(f"values has {len(values)} arrays for {self.nb} problems")
            parts = [v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
                     for v in values]
            for i, v in enumerate(parts):
                want = int(self.nnz_offsets[i + 1] - self.nnz_offsets[i])
                if v.shape != (want,):
                    raise ValueError(f"problem {i}: values has shape {v.shape}, P has {want} "
                                     "stored entries")
            values = np.concatenate(parts)
        if isinstance(values, torch.Tensor):
            v = values.detach().to(device=_device(), dtype=torch.float64).contiguous()
            if v.data_ptr() == values.data_ptr():
                v = v.clone()
        else:
            v = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float64)).to(_device())
        if v.ndim != 1 or v.numel() != self.nnz:
            raise ValueError(f"values must have the {self.nnz} stored entries of the stacked P, "
                             f"got shape {tuple(v.shape)}")
        return v

    def _tick(self, name, t0):
        import time

        import torch
        if not self.profile:
            return t0
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        self.phases[name] = self.phases.get(name, 0.0) + (t1 - t0)
        return t1

    # ------------------------------------------------------------------ one step
    def _step(self, values, want_grad):
        """(losses (nb,), convs (nb, k), errs (T + 1, nb, k), dP cuda or None)."""
        import time

        import torch
        from ._lib import call, ptr, stream_ptr
        from .sparse import DeviceCSR, galerkin
        T, nu1, nu2, nb, k = self.T, self.nu1, self.nu2, self.nb, self.k
        if T < 2:
            raise ValueError(f"tot_num_loop must be >= 2 (the loss reads errs[-3]), got {T}")
        s = stream_ptr()
        if self.profile:
            torch.cuda.synchronize()
            self.phases = {}
        t0 = time.perf_counter()
        vals = self._values(values)
        Pd = DeviceCSR.from_torch(self._p_crow, self._p_col, vals, (self.n, self.nc))
        Rd = Pd.transpose()
        Ac = galerkin(Rd, self.Ad, Pd)
        Ac2 = None if self.symmetric else galerkin(Rd, self.AT, Pd)
        t0 = self._tick("upload_galerkin", t0)
        bd = BlockDense(Ac, self.coarse_offsets)
        bdT = bd if self.symmetric or not want_grad else BlockDense(Ac2, self.coarse_offsets)
        t0 = self._tick("block_inverse", t0)
        off, max_len = self._row_off_d, self.max_len

        def remove_mean(V):
            call("mlamg_remove_mean_seg_mv", ptr(V), k, k, ptr(off), nb, max_len, s)

        def norm(V, out):
            call("mlamg_norm2_seg_mv", ptr(V), k, k, ptr(off), nb, max_len, ptr(out), s)

        X = self.X0.clone()
        rec = _recorded_forward(self.Ad, Pd, Rd, self.dinv, X, T, nu1, nu2, bd.solve,
                                remove_mean, norm, (nb, k), record=want_grad)
        errs = rec["errs_d"].cpu().numpy()
        t0 = self._tick("forward", t0)
        # cotangents of every problem's history: the single call's host arithmetic, per problem
        losses = np.empty(nb)
        convs = np.empty((nb, k))
        sc = {T: np.empty((nb, k)), T - 2: np.empty((nb, k))}
        for i in range(nb):
            losses[i], convs[i], sci = _history_cotangents(errs[:, i, :], T)
            sc[T][i], sc[T - 2][i] = sci[T], sci[T - 2]
        if not want_grad:
            return losses, convs, errs, None
        # per (problem, column) factors expanded to rows on the device
        scale = {c: torch.as_tensor(v).to(X.device).index_select(0, self._row_seg_d)
                 for c, v in sc.items()}
        dP = _adjoint_sweep(self.Ad, self.AT, self.M, Pd, Rd, X, rec, scale, T, nu1, nu2,
                            bdT.solve, remove_mean)
        torch.cuda.current_stream().synchronize()  # the step's handles are released on return
        self._tick("backward", t0)
        return losses, convs, errs, dP

    # ------------------------------------------------------------------ public surface
    def loss(self, values):
        """The nb losses (numpy fp64), each bitwise amg_loss(P_i, A_i, X_i, ...)."""
        return self._step(values, False)[0]

    def loss_and_grad(self, values, return_factors=False):
        """(losses, grad): grad is the concatenated d loss_i / d P_i.data (numpy fp64; split it
        with nnz_offsets). With return_factors also convs (nb, k) and errs (T + 1, nb, k)."""
        losses, convs, errs, dP = self._step(values, True)
        grad = dP.cpu().numpy()
        return (losses, grad, convs, errs) if return_factors else (losses, grad)

    def loss_values(self, values):
        """The nb losses as an (nb,) fp64 tensor on values.device that torch autograd can
        differentiate with respect to `values` (a 1-D fp64 tensor of all stored P values): one
        torch.autograd.Function whose backward returns dP * grad_output[problem of the entry],
        so losses.sum().backward() or losses.mean().backward() trains on the batch. Once
        differentiable only."""
        import torch
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float64 \
                or values.ndim != 1:
            raise TypeError("values must be a 1-D float64 torch tensor")
        if values.requires_grad and torch.is_grad_enabled():
            return _batch_autograd_fn().apply(values, self)
        return torch.as_tensor(self.loss(values)).to(values.device)

    def _entry_seg_on(self, device):
        t = self._entry_seg_d.get(device)
        if t is None:
            t = self._entry_seg_d[device] = self._entry_seg.to(device)
        return t


_AmgLossBatchFn = None


def _batch_autograd_fn():
    global _AmgLossBatchFn
    if _AmgLossBatchFn is not None:
        return _AmgLossBatchFn
    import torch
    from torch.autograd.function import once_differentiable

    class AmgLossBatchFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values, batch):
            losses, _, _, dP = batch._step(values, True)
            ctx.save_for_backward(dP.to(values.device), batch._entry_seg_on(values.device))
            return torch.as_tensor(losses).to(values.device)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            dP, seg = ctx.saved_tensors
            return dP * grad_output.index_select(0, seg), None

    _AmgLossBatchFn = AmgLossBatchFn
    return _AmgLossBatchFn


def _refuse_batch_early(tot_num_loop, neumann_solve_fix, who):
    """The wrappers' refusals that need no look at the problems (the loss reads errs[-3] with or
    without a gradient)."""
    if neumann_solve_fix:
        raise NotImplementedError(f"{who}: " + _NEUMANN_MSG)
    if int(tot_num_loop) < 2:
        raise ValueError(f"tot_num_loop must be >= 2 (the loss reads errs[-3]), got "
                         f"{int(tot_num_loop)}")


def amg_loss_batch(Ps, As, test_vecs, tot_num_loop=5, no_prerelax=1, no_postrelax=1,
                   neumann_solve_fix=False):
    """The nb losses of the problems (A_i, P_i): AmgLossBatch built and called once."""
    _refuse_batch_early(tot_num_loop, neumann_solve_fix, "amg_loss_batch")
    B = AmgLossBatch(As, Ps, test_vecs, tot_num_loop, no_prerelax, no_postrelax)
    return B.loss(_stored_values(Ps))


def amg_loss_and_grad_batch(Ps, As, test_vecs, tot_num_loop=5, no_prerelax=1, no_postrelax=1,
                            neumann_solve_fix=False, return_factors=False):
    """(losses, grad[, convs, errs]) of the problems (A_i, P_i): AmgLossBatch built and called
    once; grad is the concatenated gradient (split it with np.cumsum of the P_i's nnz)."""
    _refuse_batch_early(tot_num_loop, neumann_solve_fix, "amg_loss_and_grad_batch")
    B = AmgLossBatch(As, Ps, test_vecs, tot_num_loop, no_prerelax, no_postrelax)
    return B.loss_and_grad(_stored_values(Ps), return_factors=return_factors)


def _stored_values(Ps):
    """Per-problem stored values of canonical prolongators, in their stored order."""
    from .sparse import DeviceCSR
    out = []
    for P in Ps:
        P = _canonical_P(P)
        P = P.to_scipy() if isinstance(P, DeviceCSR) else P
        out.append(np.asarray(P.data, dtype=np.float64))
    return out
