"""The levels of Hierarchy.pyamg_sa: pyamg's smoothed_aggregation_solver setup on the device, per
level from the symmetric strength graph through the Galerkin product (the recipe is described
in Hierarchy.pyamg_sa), and the per-level rho rule it shares with the Chebyshev smoother."""
import ctypes
import time

import numpy as np
import scipy.sparse as sp
import torch

from ._lib import call, ptr, stream_ptr
from .graph import aggregate_op_device
from .hierarchy import Level, _level_item
from .multigrid import GaussSeidel, lambda_max_dinv_a
from .sparse import DeviceCSR, _device, csr_out, galerkin, to_device_vec
from .strength import approximate_spectral_radius


def level_rho(spec, lvl, estimates, name="rho"):
    """The spectral radius to use on level `lvl`: `spec` names one of `estimates` (name -> a
    function that computes the level's value, e.g. 'lanczos', 'arnoldi'), or is a number for
    every level, or a list / tuple with one number per level."""
    if isinstance(spec, str) and spec in estimates:
        return estimates[spec]()
    r = _level_item(spec, lvl) if isinstance(spec, (list, tuple)) else spec
    if r is None:
        raise ValueError(f"no {name} given for level {lvl}")
    return float(r)


def _improve_candidates(L, Bv, lvl, iterations):
    """pyamg's improve_candidates (level 0 only): symmetric block Gauss-Seidel sweeps on
    A B = 0. The same sweep later smooths this level: one handle. Sets L.B."""
    if lvl == 0 and iterations > 0:
        L.gs = GaussSeidel(L.A, "symmetric", block=True)
        L.gs.sweep(Bv, torch.zeros_like(Bv), int(iterations))
    L.B = Bv


def _empty_level(L, cpts, Bv, lvl, improve_iterations, rho, omega):
    """The level when standard aggregation finds no aggregate: an n x 1 empty AggOp (pyamg's
    standard_aggregation return), T = 0, B_c = [0], P = 0 (n x 1), R = P^T, A_c = [[0]]. The
    level keeps its symmetric block Gauss-Seidel smoother (pyamg still smooths it; for the
    operators this happens on — no off-diagonal couplings — the sweep is an exact solve).
    Fills L and returns (A_c, B_c)."""
    n = L.A.shape[0]
    dev = _device()
    L.Agg = DeviceCSR.from_scipy(sp.csr_matrix((n, 1)))
    L.seeds = cpts[:0]
    L.n_seeds = 1
    _improve_candidates(L, Bv, lvl, improve_iterations)
    dinv = torch.empty(n, dtype=torch.float64, device=dev)
    call("mlamg_diag_pinv", L.A.handle, ptr(dinv), stream_ptr())
    L.lam = level_rho(rho, lvl, {
        # rho(D^-1 A) of an operator without off-diagonal couplings: 1 where a_ii != 0
        "lanczos": lambda: 1.0 if bool((dinv != 0).any()) else 0.0,
        # pyamg's estimate (draws from numpy's global generator)
        "arnoldi": lambda: approximate_spectral_radius(
            csr_out("mlamg_csr_scale_rows", L.A.handle, ptr(dinv), 0))})
    L.omega = omega / L.lam if L.lam else 0.0
    L.P = DeviceCSR.from_scipy(sp.csr_matrix((n, 1)))
    L.R = DeviceCSR.from_scipy(sp.csr_matrix((1, n)))
    L.dinv = dinv
    return (DeviceCSR.from_scipy(sp.csr_matrix((1, 1))),
            torch.zeros(1, dtype=torch.float64, device=dev))


def build_levels(H, A_dev, B, *, max_levels, max_coarse, theta, omega, improve_iterations, rho,
                 verbose):
    """Append Hierarchy.pyamg_sa's levels of A_dev to H (its keywords, as given there) and set
    H.Ac, H.B_coarse and H.galerkin_s. Returns the seconds spent per setup phase."""
    dev = _device()
    n0 = A_dev.shape[0]
    if B is None:
        Bv = torch.ones(n0, dtype=torch.float64, device=dev)
    else:
        Bn = np.asarray(B, dtype=np.float64)
        if Bn.size != n0:
            raise NotImplementedError("one near-nullspace candidate (B of shape (n, 1))")
        Bv = to_device_vec(Bn.reshape(-1)).clone()
    tm = {"strength": 0.0, "aggregation": 0.0, "candidates": 0.0, "rho": 0.0,
          "prolongator": 0.0, "galerkin": 0.0}
    H.galerkin_s = []
    while A_dev.shape[0] > max_coarse and len(H.levels) + 1 < max_levels:
        n = A_dev.shape[0]
        lvl = len(H.levels)
        L = Level(A_dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        C = csr_out("mlamg_symmetric_strength", A_dev.handle, float(theta))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        agg = torch.empty(n, dtype=torch.int32, device=dev)
        cpts = torch.empty(n, dtype=torch.int32, device=dev)
        k, rounds = ctypes.c_int64(), ctypes.c_int32()
        call("mlamg_standard_aggregation", C.handle, ptr(agg), ptr(cpts), ctypes.byref(k),
             ctypes.byref(rounds), stream_ptr())
        del C
        k = int(k.value)
        L.agg_col = agg
        L.bf_sweeps = int(rounds.value)
        if k == 0:
            # no node has an off-diagonal strength entry (a diagonal or fully decoupled
            # operator): pyamg's standard_aggregation returns an n x 1 empty AggOp, so
            # T = 0, B_c = 0, P = 0 and A_c = [[0]], whose pinv is 0 (a zero coarse
            # correction); the level keeps its smoother
            A_dev, Bv = _empty_level(L, cpts, Bv, lvl, improve_iterations, rho, omega)
            H.galerkin_s.append(0.0)
            H.levels.append(L)
            continue
        L.Agg = aggregate_op_device(agg, k)
        L.seeds = cpts[:k]
        L.n_seeds = k
        t2 = time.perf_counter()
        _improve_candidates(L, Bv, lvl, improve_iterations)
        h = ctypes.c_void_p()
        Bc = torch.empty(k, dtype=torch.float64, device=dev)
        call("mlamg_fit_candidates", L.Agg.handle, ptr(Bv), 1e-10, ctypes.byref(h), ptr(Bc),
             stream_ptr())
        T = DeviceCSR(h)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        dinv = torch.empty(n, dtype=torch.float64, device=dev)
        call("mlamg_diag_pinv", A_dev.handle, ptr(dinv), stream_ptr())
        DinvA = csr_out("mlamg_csr_scale_rows", A_dev.handle, ptr(dinv), 0)

        def lanczos():
            # pyamg's own estimate is a 15-step Arnoldi value to a relative 1e-2
            # (approximate_spectral_radius's tol); 1e-6 is far tighter
            lam, L.lanczos_iters = lambda_max_dinv_a(A_dev, tol=1e-6)
            return abs(lam)
        L.lam = level_rho(rho, lvl, {"lanczos": lanczos,
                                     "arnoldi": lambda: approximate_spectral_radius(DinvA)})
        t4 = time.perf_counter()
        L.omega = omega / L.lam
        cvec = torch.full((n,), L.omega, dtype=torch.float64, device=dev)
        DinvA = csr_out("mlamg_csr_scale_rows", DinvA.handle, ptr(cvec), 0)
        M = DinvA @ T
        del DinvA
        L.P = csr_out("mlamg_csr_sub", T.handle, M.handle)
        del M, T
        L.R = L.P.transpose()
        L.dinv = dinv
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        A_next = galerkin(L.R, A_dev, L.P)
        torch.cuda.synchronize()
        t6 = time.perf_counter()
        for key, dt in (("strength", t1 - t0), ("aggregation", t2 - t1),
                        ("candidates", t3 - t2), ("rho", t4 - t3),
                        ("prolongator", t5 - t4), ("galerkin", t6 - t5)):
            tm[key] += dt
        H.galerkin_s.append(round(t6 - t5, 4))
        H.levels.append(L)
        if verbose:
            print(f"[mlamg pyamg_sa] level {lvl}: n={n} nnz={A_dev.nnz} aggregates={k} "
                  f"rounds={L.bf_sweeps} rho={L.lam:.6g} P nnz={L.P.nnz} -> "
                  f"n_c={A_next.shape[0]} nnz_c={A_next.nnz}", flush=True)
        A_dev = A_next
        Bv = Bc
    H.Ac = A_dev
    H.B_coarse = Bv
    call("mlamg_scratch_trim", None)
    return tm
