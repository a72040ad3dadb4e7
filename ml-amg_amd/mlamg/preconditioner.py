"""PETSc python-PC mirror of ns/preconditioner/MLAMG.py (and the multilevel PyAMG PC), plus the
package-level precondition()/solve() entry points.

Reference surface (ns/preconditioner/MLAMG.py):
  class MLAMG(PCBase): initialize(pc) :30, update(pc) :126, apply(pc, X, Y) :199,
  applyTranspose :214, view :218; options '<prefix>mlamg_amg_rtol' (1e-8, :64),
  'mlamg_jacobi_weight' (2/3, :66); apply runs amg_2_v (:148-197) from x0 = np.random.normal
  (:209) with the weighted-Jacobi smoother until ||b - A x||_2 <= amg_rtol, at most 500 cycles.

What differs: the reference always builds P with a learned GNN (greedy C/F splitting, then
InterpolationNetwork, :105-120) and fails without its trained weights, which are not shipped. Here
that setup runs when the option 'mlamg_pnet_model' names a saved state_dict (with
'mlamg_greedy_theta', default 0.56, :65-67): mlamg.greedy.greedy_coarsening on the host,
mlamg.interp.InterpolationNetwork.forward_mat on the device (torch_geometric's layers restated,
parity with it unpinned: see mlamg/interp.py), then the Galerkin product and the coarse
factorisation of Hierarchy.two_level. Without the option P is the smoothed-aggregation
prolongator of seeded Bellman-Ford aggregates, built on the GPU (option 'mlamg_alpha', default
0.1), or any P handed in via `MLAMG.set_prolongator`. The cycle, stopping rule and I/O contract
are the reference's. The PC works with petsc4py when present and
with any duck-typed object offering getOperators()/getOptionsPrefix() otherwise (no PETSc here).
"""
from __future__ import annotations

import traceback

import numpy as np
import scipy.sparse as sp
import torch

from .hierarchy import Hierarchy
from .sparse import to_device_vec


class _Options:
    """PETSc.Options stand-in: a dict; petsc4py's Options is used when importable."""

    store = {}

    def __init__(self):
        try:  # pragma: no cover - petsc4py is not installed in this image
            from petsc4py import PETSc
            self._petsc = PETSc.Options()
        except Exception:
            self._petsc = None

    def getScalar(self, key, default):
        if self._petsc is not None:  # pragma: no cover
            return self._petsc.getScalar(key, default)
        return float(self.store.get(key, default))

    def getInt(self, key, default):
        if self._petsc is not None:  # pragma: no cover
            return self._petsc.getInt(key, default)
        return int(self.store.get(key, default))

    def getString(self, key, default):
        if self._petsc is not None:  # pragma: no cover
            return self._petsc.getString(key, default)
        return str(self.store.get(key, default))

    def getBool(self, key, default):
        if self._petsc is not None:  # pragma: no cover
            return self._petsc.getBool(key, default)
        v = self.store.get(key, default)
        if isinstance(v, str):
            return v.strip().lower() in ("1", "true", "yes", "on")
        return bool(v)


def _csr_from_pc(pc):
    _, P = pc.getOperators()
    if hasattr(P, "getValuesCSR"):
        row, col, val = P.getValuesCSR()
        return sp.csr_matrix((val, col, row))
    return sp.csr_matrix(P)


class MLAMG:
    """Two-level weighted-Jacobi AMG preconditioner (MLAMG.py:27-222) on the MI355X."""

    _prefix = "mlamg_"

    def __init__(self):
        self._P_user = None

    # ------------------------------------------------------------------ PCBase protocol
    def initialize(self, pc):
        try:
            self._initialize(pc)
        except Exception as e:
            traceback.print_exc()
            raise e

    def _initialize(self, pc):
        prefix = pc.getOptionsPrefix() if hasattr(pc, "getOptionsPrefix") else ""
        prefix = (prefix or "") + self._prefix
        opts = _Options()
        self.amg_rtol = opts.getScalar(f"{prefix}amg_rtol", 1e-8)
        self.jacobi_weight = opts.getScalar(f"{prefix}jacobi_weight", 2.0 / 3.0)
        self.alpha = opts.getScalar(f"{prefix}alpha", 0.1)
        self.max_iter = opts.getInt(f"{prefix}max_iter", 500)
        self.coarsening_theta = opts.getScalar(f"{prefix}greedy_theta", 0.56)
        self.pnet_model_fname = opts.getString(f"{prefix}pnet_model", "")
        self.update(pc)

    def set_prolongator(self, P):
        """Use a given interpolation operator (e.g. a learned P) instead of SA-on-BF."""
        self._P_user = P

    def update(self, pc):
        try:
            self._createAmgSolver(pc)
        except Exception as e:
            traceback.print_exc()
            raise e

    def _createAmgSolver(self, pc):
        A = _csr_from_pc(pc)
        self.A = A
        if self._P_user is not None:
            P = self._P_user
        elif getattr(self, "pnet_model_fname", ""):
            P = self._learned_P(A)
        else:
            H = Hierarchy.build(A, alpha=self.alpha, max_levels=2, max_coarse=0,
                                jacobi_weight=self.jacobi_weight, finalize=False)
            P = H.levels[0].P
        self.H = Hierarchy.two_level(A, P, omega=self.jacobi_weight)

    def _learned_P(self, A):
        """The reference's setup (MLAMG.py:105-120): load the P-net, greedy C/F splitting,
        forward_mat."""
        from .greedy import greedy_coarsening
        from .interp import InterpolationNetwork
        self.P_net = InterpolationNetwork()
        try:
            state_dict = torch.load(self.pnet_model_fname, weights_only=True)
            self.P_net.model.load_state_dict(state_dict)
            self.P_net.eval()
        except Exception as e:
            raise RuntimeError(f'Could not load PNet model "{self.pnet_model_fname}": {e}')
        self.P_net.to(torch.device("cuda", torch.cuda.current_device()))
        _, F, C = greedy_coarsening(A, self.coarsening_theta)
        self.P_amg = self.P_net.forward_mat(A, C, F)
        return self.P_amg

    def apply(self, pc, X, Y):
        try:
            self._apply(pc, X, Y)
        except Exception as e:
            traceback.print_exc()
            raise e

    def _apply(self, pc, X, Y):
        b = X.array_r if hasattr(X, "array_r") else np.asarray(X)
        x = np.random.normal(size=self.A.shape[1])  # MLAMG.py:209 (global RNG, unseeded)
        bd = to_device_vec(b)
        xd = to_device_vec(x).clone()
        self.H.cycle(bd, xd, self.max_iter, tol=self.amg_rtol)
        out = xd.cpu().numpy()
        if hasattr(Y, "setArray"):
            Y.setArray(out)
        else:
            Y[...] = out

    def applyTranspose(self, pc, X, Y):
        print('PyAMG applyTranspose!')  # reference behaviour: a no-op (MLAMG.py:214-216)

    def view(self, pc, viewer=None):
        if viewer is not None:
            viewer.printfASCII('MLAMG (MI355X) Solver:\n')
            viewer.printfASCII(f' levels: {self.H.n_levels}\n')
            viewer.printfASCII(f' amg rtol: {self.amg_rtol}\n')


class MultilevelPC(MLAMG):
    """The PyAMG PC (ns/preconditioner/PyAMG.py:13-130) on the MI355X.

    Setup (:79-100): `pyamg.aggregation.smoothed_aggregation_solver(P, max_levels=...)` (:94)
    with at most '<prefix>pyamg_amg_max_levels' levels (default 10, :53), built on the device
    with pyamg's default recipe (Hierarchy.pyamg_sa: symmetric strength, standard aggregation,
    candidate improvement by symmetric block Gauss-Seidel, fit_candidates, Jacobi-smoothed P
    with omega 4/3 / rho(D^-1 A), max_coarse 10, pinv coarse solve, symmetric block Gauss-Seidel
    V(1,1)); pyamg itself is absent, so parity is unpinned (bitwise the oracle's restatement).
    Option '<prefix>pyamg_amg_smoother' = 'chebyshev' (default 'block_gauss_seidel') smooths with
    pyamg's polynomial smoother of degree '<prefix>pyamg_amg_chebyshev_degree' (default 3)
    instead: presmoother = postsmoother = ('chebyshev', {'degree': d}).
    Option '<prefix>pyamg_amg_recipe' = 'mlamg_sa' selects this package's own SA hierarchy
    instead (seeded Bellman-Ford aggregates, Jacobi smoothing, dense coarsest level).
    Apply (:118-120), `Amg.solve(b, tol=amg_rtol, accel='gmres' if amg_precondition_with_gmres
    else None)`: zero initial guess and a tolerance relative to ||b|| (pyamg's solve scales tol
    by ||b||, and its default maxiter is 100).
      * with GMRES (the default, :54): pyamg.krylov.gmres's default Householder GMRES on the
        device, preconditioned by one V-cycle (Hierarchy.gmres_householder): ONE outer cycle
        (no restart value) of at most maxiter = 100 inner steps, stopping when the
        preconditioned residual ||M r|| < tol ||M b||. Option
        '<prefix>pyamg_amg_gmres_orthog' = 'mgs' selects the restarted-MGS GMRES
        (Hierarchy.gmres, scipy's algorithm) with the same budget and stop test instead;
      * without: stationary V-cycles from x = 0 until ||b - A x|| <= amg_rtol ||b||, at most 100.
    """

    _prefix = "pyamg_"
    PYAMG_MAXITER = 100  # pyamg multilevel_solver.solve default

    def _initialize(self, pc):
        prefix = ((pc.getOptionsPrefix() if hasattr(pc, "getOptionsPrefix") else "") or "")
        opts = _Options()
        self.amg_precon_gmres = opts.getBool(
            f"{prefix}{self._prefix}amg_precondition_with_gmres", True)
        self.gmres_orthog = opts.getString(
            f"{prefix}{self._prefix}amg_gmres_orthog", "householder")
        if self.gmres_orthog not in ("householder", "mgs"):
            raise ValueError(f"unknown amg_gmres_orthog {self.gmres_orthog!r} "
                             "(householder, mgs)")
        super()._initialize(pc)

    def _createAmgSolver(self, pc):
        A = _csr_from_pc(pc)
        self.A = A
        opts = _Options()
        prefix = ((pc.getOptionsPrefix() if hasattr(pc, "getOptionsPrefix") else "") or "")
        levels = opts.getInt(f"{prefix}{self._prefix}amg_max_levels", 10)
        recipe = opts.getString(f"{prefix}{self._prefix}amg_recipe", "pyamg_sa")
        smoother = opts.getString(f"{prefix}{self._prefix}amg_smoother", "block_gauss_seidel")
        degree = opts.getInt(f"{prefix}{self._prefix}amg_chebyshev_degree", 3)
        if smoother not in ("block_gauss_seidel", "chebyshev"):
            raise ValueError(f"unknown amg_smoother {smoother!r} (block_gauss_seidel, chebyshev)")
        if recipe == "pyamg_sa":
            if smoother == "chebyshev":
                self.H = Hierarchy.pyamg_sa(A, max_levels=levels,
                                            smoother=("chebyshev", {"degree": degree}))
            else:
                self.H = Hierarchy.pyamg_sa(A, max_levels=levels)
        elif recipe == "mlamg_sa":
            self.H = Hierarchy.build(A, alpha=self.alpha, max_levels=levels,
                                     jacobi_weight=self.jacobi_weight)
            if smoother == "chebyshev":
                self.H._set_chebyshev({"degree": degree}, "arnoldi")
        else:
            raise ValueError(f"unknown amg_recipe {recipe!r} (pyamg_sa, mlamg_sa)")

    def _apply(self, pc, X, Y):
        b = X.array_r if hasattr(X, "array_r") else np.asarray(X)
        b = np.asarray(b, dtype=np.float64)
        if self.amg_precon_gmres:
            if self.gmres_orthog == "householder":
                out = self.H.gmres_householder(b, tol=self.amg_rtol, maxiter=self.PYAMG_MAXITER)
            else:
                out = self.H.gmres(b, rtol=self.amg_rtol, restart=self.PYAMG_MAXITER, maxiter=1)
        else:
            normb = float(np.linalg.norm(b))
            tol = self.amg_rtol * normb if normb != 0 else self.amg_rtol
            bd = to_device_vec(b)
            xd = torch.zeros_like(bd)
            if normb > tol:  # pyamg: while residuals[-1] > tol (||r_0|| = ||b|| at x = 0)
                self.H.cycle(bd, xd, self.PYAMG_MAXITER, tol=tol)
            out = xd.cpu().numpy()
        if hasattr(Y, "setArray"):
            Y.setArray(out)
        else:
            Y[...] = out


# ---------------------------------------------------------------------- package-level API
def setup(A, **kw):
    """Build the device hierarchy once (Hierarchy.build keywords)."""
    return Hierarchy.build(A, **kw)


def precondition(H, b):
    """Action of one V-cycle from x = 0 on b (numpy in -> numpy out, tensor in -> tensor out)."""
    return H.precondition(b)


def solve(A_or_H, b, x0=None, tol=1e-8, maxiter=500, return_history=False, **kw):
    """V-cycle iteration until ||b - A x||_2 <= tol (absolute, MLAMG.py:194)."""
    H = A_or_H if isinstance(A_or_H, Hierarchy) else Hierarchy.build(A_or_H, **kw)
    return H.solve(b, x0=x0, tol=tol, maxiter=maxiter, return_history=return_history)
