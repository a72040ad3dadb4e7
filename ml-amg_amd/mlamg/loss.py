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
"""
from __future__ import annotations

import numpy as np

__all__ = ["amg_loss", "amg_loss_and_grad", "amg_loss_values", "loss_from_errs"]

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


def _loss_and_grad_device(P, A, test_vecs, tot_num_loop, no_prerelax, no_postrelax):
    """(loss, dP as a cuda tensor in the stored order of the canonical P, convs, errs)."""
    import ctypes

    import torch
    from ._lib import call, ptr, stream_ptr
    from .hierarchy import Hierarchy, csr_symmetric
    from .sparse import DeviceCSR, mv_block, to_device_vec
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
    nc = Pd.shape[1]
    dev = X.device
    s = stream_ptr()

    def block(rows, *lead):
        return torch.empty(lead + (rows, k), dtype=torch.float64, device=dev)

    def coarse_solve(rhs, out):
        # the forward's solver; PCG was chosen because A_H is symmetric, so it is A_H^-T too
        if H.pcg is not None:
            call("mlamg_pcg_solve_mv", H.pcg, ptr(rhs), k, ptr(out), k, k, s)
        else:
            call("mlamg_dense_solve_mv", H.dense, ptr(rhs), k, ptr(out), k, k, s)

    # ---- recorded forward: the block cycle's own steps (csrc/hier.hip mlamg_hier_vcycle_mv)
    ncyc = T + 1
    X2 = block(n, ncyc)    # x after the coarse correction, per cycle
    E = block(nc, ncyc)    # the coarse correction e, per cycle
    X4 = {}                # x after the mean removal, for the two cycles the loss reads
    tmp, r, bc = block(n), block(n), block(nc)
    errs_d = torch.empty((ncyc, k), dtype=torch.float64, device=dev)
    for c in range(ncyc):
        if nu1:
            call("mlamg_jacobi_mv", Ad.handle, ptr(dinv), None, 0, ptr(X), k, ptr(tmp), k, k,
                 nu1, s)
        call("mlamg_residual_mv", Ad.handle, None, 0, ptr(X), k, ptr(r), k, k, None, s)
        call("mlamg_restrict_mv", Rd.handle, ptr(r), k, ptr(bc), k, k, s)
        coarse_solve(bc, E[c])
        call("mlamg_prolong_add_mv", Pd.handle, ptr(E[c]), k, ptr(X), k, k, s)
        X2[c].copy_(X)
        if nu2:
            call("mlamg_jacobi_mv", Ad.handle, ptr(dinv), None, 0, ptr(X), k, ptr(tmp), k, k,
                 nu2, s)
        call("mlamg_remove_mean_mv", ptr(X), k, n, k, s)
        call("mlamg_norm2_mv", ptr(X), k, n, k, ptr(errs_d[c]), s)
        if c in (T, T - 2):
            X4[c] = X.clone()
    errs = errs_d.cpu().numpy()
    H.check_coarse()  # a PCG breakdown in the forward: CoarseSolveError
    loss, convs = loss_from_errs(errs)

    # ---- cotangents of the error history (host arithmetic on k numbers)
    w = np.exp(convs - convs.max())
    w = w / w.sum()
    dconv = w * (1.0 + convs - loss)
    scale = {T: dconv * convs / (2.0 * errs[T]) / errs[T],
             T - 2: -dconv * convs / (2.0 * errs[T - 2]) / errs[T - 2]}
    scale = {c: torch.as_tensor(v, dtype=torch.float64).to(dev) for c, v in scale.items()}

    # ---- adjoint operators, built once
    h = ctypes.c_void_p()
    call("mlamg_csr_scale_rows", Ad.handle, ptr(dinv), 0, ctypes.byref(h), s)
    DA = DeviceCSR(h)
    M = DA.transpose()  # (D A)^T: one adjoint Jacobi sweep is g - M g
    del DA
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

    def adjoint_jacobi(g, g2, nu):
        for _ in range(nu):
            g2.copy_(g)
            M.matmat(g, out=g2, alpha=-1.0, beta=1.0)
            g, g2 = g2, g
        return g, g2

    # ---- backward sweep over the cycles
    g = torch.zeros((n, k), dtype=torch.float64, device=dev)
    g2, q, ax2 = tmp, r, X  # the forward's work blocks, free now
    t, lam = bc, block(nc)
    dP = torch.zeros(Pd.nnz, dtype=torch.float64, device=dev)
    for c in range(T, -1, -1):
        if c in scale:
            g.addcmul_(X4[c], scale[c])
        call("mlamg_remove_mean_mv", ptr(g), k, n, k, s)
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
