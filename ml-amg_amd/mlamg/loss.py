"""The reference's AMG loss of a prolongator, forward evaluation on the device.

Reference: ns/model/loss.py:32-96 (amg_loss). It scores an interpolation operator P by running
tot_num_loop + 1 two-level cycles on a block of k test vectors with a zero right-hand side
(pre-relaxation, coarse-grid correction, post-relaxation, mean removal: loss.py:70-89), records
||x_j||_2 of every column after each cycle (loss.py:90) and turns the last three rows of that
history into per-column convergence factors convs = (errs[-1] / errs[-3]) ** (1/2) and the
softmax-weighted loss softmax(convs) @ convs (loss.py:92-94).

Here the cycles run through the block V-cycle of the library (Hierarchy.cycle_multi,
mlamg_hier_vcycle_mv): every operator is streamed once for all k columns.

Differences from the reference, all stated:
  * fp64 throughout. The reference holds x, A and P in fp32 and only solves the coarse system in
    fp64 (loss.py:54,59,79). torch_sparse / torch_sparse_solve, which the reference needs, are
    not available to this project's tests, so its fp32 numbers are parity-unpinned: the tests pin
    the history bit for bit to the library's single-vector cycle and to an fp64 numpy/scipy
    restatement of loss.py:48-96 within the project's SuperLU-versus-dense bounds.
  * forward evaluation only: no autograd through the cycle.
  * neumann_solve_fix=True (the Lagrange-row coarse system, loss.py:11-30,66-67,76-82) is not
    implemented and raises NotImplementedError.
"""
from __future__ import annotations

import numpy as np

__all__ = ["amg_loss", "loss_from_errs"]


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
    Returns the loss (float); with return_factors=True, (loss, convs, errs) with errs the
    (tot_num_loop + 1, k) history of ||x_j||_2 after each cycle."""
    if neumann_solve_fix:
        raise NotImplementedError("amg_loss: neumann_solve_fix=True (the Lagrange-row coarse "
                                  "system of ns/model/loss.py:11-30) is not implemented")
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
