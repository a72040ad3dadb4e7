"""Device AMG hierarchy: setup on the GPU and the V-cycle executor (mlamg_hier_*).

Setup per level follows the reference's aggregation-based SA recipe, all on the device:
  C = strength(A)                                    utils/common.py:25-31 ('invabs', 'abs', 'unit',
                                                     'evolution', 'olson')
  seeds = RandomState(seed).permutation(n)[:ceil(alpha*n)]       graph.py:230-231; evaluate_dataset.py:80-85
  (dist, label) = Bellman-Ford(C, seeds)            graph.py:7-53   (or Lloyd: graph.py:156-239)
  Agg = aggregate operator(label)                   graph.py:56-86
  omega = (4/3)/lambda_max(Dinv A);  P = (I - omega Dinv A) Agg    multigrid.py:102-108
  R = P^T;  A_c = (R A) P                            multigrid.py:165
until n <= max_coarse; the last operator is inverted densely (multigrid.py:168 factorized).
The cycle is the Jacobi V(1,1) of ns/preconditioner/MLAMG.py:143-197 applied recursively.

Seeds are RandomState(seed).permutation(n)[:k] bit for bit, the reference seeding (numpy's
MT19937 draws on the host, the shuffle's first k positions resolved on the device: graph.
legacy_permutation); with sort_seeds=True (default for the multilevel solver) they are sorted so that
coarse unknowns follow the fine ordering (better locality, contiguous ownership per GPU).

This module holds the Hierarchy handle: its cycling and solver methods, the coarse-solver
choice and two_level. The per-level setup loops live in mlamg/sa_setup.py (Hierarchy.build,
the recipe above) and mlamg/pyamg_setup.py (Hierarchy.pyamg_sa), the SpMV format search that
apply_formats runs in mlamg/autotune.py.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np
import torch

from . import _lib, autotune
from ._lib import MLAMG_EUNSUPPORTED, MlamgError, _tol_arg, call, ptr, stream_ptr
from .sparse import DeviceCSR, as_device, csr_out, galerkin, to_device_vec

STRENGTH_MODES = {"abs": 0, "invabs": 1, "unit": 2, "same": 3}


def strength(A_dev, mode="invabs", rho=None):
    """Strength graph of a device operator: the elementwise measures of utils/common.py:26,28,29
    or the evolution measures of :27,30 ('evolution', 'olson'; rho(D^-1 A) = rho, default the
    device Lanczos value)."""
    if mode in ("evolution", "olson"):
        from .strength import evolution_device
        return evolution_device(A_dev, mode, rho=rho)
    return csr_out("mlamg_strength", A_dev.handle, STRENGTH_MODES[mode])


class CoarseSolveError(RuntimeError):
    """The coarsest solve cannot be done as asked (PCG on a non-symmetric operator too large
    for the dense solver) or a PCG coarse solve broke down (operator not positive definite)."""
    code = MLAMG_EUNSUPPORTED


def csr_symmetric(M, rtol=0.0):
    """True when the device CSR M is symmetric to `rtol` (mlamg_csr_symmetric)."""
    ok = ctypes.c_int()
    call("mlamg_csr_symmetric", M.handle, float(rtol), ctypes.byref(ok), stream_ptr())
    return bool(ok.value)


class Level:
    __slots__ = ("A", "dinv", "P", "R", "Agg", "omega", "lam", "lanczos_iters", "n_seeds",
                 "bf_sweeps", "seeds", "gs", "labels", "agg_col", "B", "sa_prolong", "poly",
                 "rho_A")

    def __init__(self, A):
        self.A = A
        self.dinv = None
        self.P = self.R = self.Agg = None
        self.omega = self.lam = None
        self.lanczos_iters = 0
        self.n_seeds = 0
        self.bf_sweeps = 0
        self.seeds = None
        self.gs = None
        self.labels = None  # per-node aggregate seed (node id, -1 none) when built by BF
        self.agg_col = None  # per-node aggregate column (int32 device tensor, -1 none)
        self.B = None  # near-nullspace candidate fitted at this level (pyamg_sa)
        self.sa_prolong = False  # P = (I - omega D^-1 A) Agg formed here (mlamg_sa_smoother)
        self.poly = None  # polynomial smoother in use (multigrid.Polynomial), else None
        self.rho_A = None  # rho(A) its Chebyshev coefficients were made for


def _level_item(spec, lvl):
    """The level-`lvl` entry of a per-level specification (None, one item = level 0, or a
    list / tuple of items)."""
    if spec is None:
        return None
    if isinstance(spec, (list, tuple)):
        return spec[lvl] if lvl < len(spec) else None
    return spec if lvl == 0 else None


def _smoother_spec(smoother):
    """(name, options) of a pyamg-style smoother argument: a name or a (name, dict) pair."""
    if isinstance(smoother, str):
        return smoother, {}
    if isinstance(smoother, (tuple, list)) and len(smoother) == 2 and isinstance(smoother[0], str):
        return smoother[0], dict(smoother[1] or {})
    raise ValueError(f"smoother must be a name or a (name, options) pair, got {smoother!r}")


CHEBYSHEV_DEFAULTS = {"degree": 3, "iterations": 1, "lower_bound": 1.0 / 30.0, "upper_bound": 1.1}


def _chebyshev_options(opts):
    """pyamg's setup_chebyshev keywords with their defaults; anything else is refused."""
    extra = set(opts) - set(CHEBYSHEV_DEFAULTS)
    if extra:
        raise NotImplementedError(f"chebyshev smoother options {sorted(extra)}")
    o = dict(CHEBYSHEV_DEFAULTS, **opts)
    if int(o["degree"]) < 1 or int(o["iterations"]) < 1:
        raise ValueError("chebyshev degree and iterations must be >= 1")
    return o


def rhs_arg(b):
    """The right-hand side handed to mlamg_hier_vcycle: None when every entry of b is +0.0
    (bit pattern 0, so -0.0 does not count) — the reference's convergence-factor problems
    (utils/common.py:74, utils/evaluate_dataset.py:92: b = zeros). The fine-level kernels then
    take b = +0.0 instead of streaming a vector of zeros; the results are the same bits. One
    reduction over b per call (no per-cycle cost)."""
    if b is None:
        return None
    if b.numel() and bool(torch.count_nonzero(b.reshape(-1).contiguous().view(torch.int64))):
        return b
    return None


class Hierarchy:
    """A multilevel (or two-level) smoothed-aggregation hierarchy resident on the GPU."""

    def __init__(self):
        self.levels = []
        self.Ac = None
        self.dense = None
        self.handle = None
        self.recipe = "mlamg_sa"  # Hierarchy.build / two_level; "pyamg_sa" from pyamg_sa()
        self.jacobi_weight = 2.0 / 3.0
        self.nu_pre = 1
        self.nu_post = 1
        self.timings = {}
        self.pcg = None
        self.inner = None
        self.coarse_gmres = False  # coarsest solve by GMRES + inner hierarchy (_make_coarse_gmres)
        self._breakdowns_seen = 0
        self._factored = {}
        self.poly_iterations = 1
        self._recipe_poly = None  # (per-level coefficients, iterations) of a Chebyshev recipe

    # ------------------------------------------------------------------ construction
    @classmethod
    def two_level(cls, A, P, omega=2.0 / 3.0, nu_pre=1, nu_post=1, dinv_w=None,
                  smoother="jacobi", norm="residual", coarse="auto", degree=3,
                  smoother_rho="arnoldi"):
        """Two-level cycle with a given P: MLAMG.amg_2_v (ns/preconditioner/MLAMG.py:120-122,
        smoother='jacobi') or multigrid.amg_2_v (multigrid.py:111-210, smoother='gauss_seidel';
        norm='x' records ||x||_2 per cycle, the error_tol mode). coarse='dense' forces the
        dense inverse (up to DENSE_LIMIT rows) where 'auto' would take PCG; coarse='gmres'
        the GMRES coarse solve (any A_c; Hierarchy._make_coarse_gmres). smoother='chebyshev':
        pyamg's polynomial smoother of the given degree for rho(A) = smoother_rho ('arnoldi':
        pyamg's approximate_spectral_radius, or a number), one iteration per sweep."""
        from .multigrid import GaussSeidel
        H = cls()
        H.jacobi_weight = omega
        tm, t0 = {}, time.perf_counter()
        L = Level(as_device(A))
        L.P = as_device(P)
        L.R = L.P.transpose()
        L.dinv = L.A.diag_inv(omega) if dinv_w is None else to_device_vec(dinv_w)
        H.levels.append(L)
        torch.cuda.synchronize()
        tm["upload"], t0 = time.perf_counter() - t0, time.perf_counter()
        H.Ac = galerkin(L.R, L.A, L.P)
        torch.cuda.synchronize()
        tm["galerkin"], t0 = time.perf_counter() - t0, time.perf_counter()
        n_c = H.Ac.shape[0]
        if coarse == "dense" and n_c > cls.DENSE_LIMIT:
            raise CoarseSolveError(f"coarse operator of {n_c} rows: the dense solver is limited "
                                   f"to {cls.DENSE_LIMIT} rows")
        if coarse not in ("auto", "dense", "gmres"):
            raise ValueError(f"unknown coarse solver {coarse!r}")
        H._finalize(nu_pre, nu_post,
                    dense_max=n_c if coarse == "dense" else cls.TWO_LEVEL_DENSE_MAX,
                    coarse="gmres" if coarse == "gmres" else None)
        torch.cuda.synchronize()
        tm["coarse_solver"], t0 = time.perf_counter() - t0, time.perf_counter()
        if smoother == "gauss_seidel":
            L.gs = GaussSeidel(L.A)
            call("mlamg_hier_set_level_smoother", H.handle, 0, L.gs.handle)
            torch.cuda.synchronize()
            tm["gauss_seidel"] = time.perf_counter() - t0
        elif smoother == "chebyshev":
            H._set_chebyshev({"degree": degree}, smoother_rho)
            torch.cuda.synchronize()
            tm["chebyshev"] = time.perf_counter() - t0
        elif smoother != "jacobi":
            raise ValueError(f"unknown smoother {smoother!r}")
        H.timings = tm
        if norm not in ("residual", "x"):
            raise ValueError(f"unknown norm {norm!r}")
        call("mlamg_hier_set_norm", H.handle, 0 if norm == "residual" else 1)
        return H

    # operators whose mean row has at least this many entries use the lane-parallel CSR-vector
    # family (canonical order, one result for every width); shorter rows use the exact-order
    # (scipy) family. A rule on the matrix, not a timing: measured on the C4 hierarchy
    # (tools/coarse_formats.py) the vector kernels win from R_2 (357 entries per row: 18 vs
    # 34 us) up and lose below (A_2, 187 per row: 79 vs 54 us).
    VEC_MIN_MEAN_ROW = 256

    @staticmethod
    def clear_tune_cache():
        """Forget the autotune's decisions: the next apply_formats times every operator."""
        autotune.clear()

    def apply_formats(self, fine_format="autotune", coarse_format="auto", vec_min_row=None,
                      first_level=0):
        """Choose the SpMV kernel of every operator.

        The candidates of one operator all compute the same bits, so the autotune — a timing
        decision — cannot change any result:
          * mean row length < vec_min_row (default VEC_MIN_MEAN_ROW): the exact-order family,
            scipy's left-to-right order (CSR-stream, SELL-64[-sigma], dictionary SELL,
            gather-sorted CSR-stream, row-pair patterns, long-row tiles) — bitwise A @ x;
          * otherwise (levels >= 1 only; coarse_format='auto'): the CSR-vector family, widths
            64..512 in one canonical lane-parallel order (oracle.c vec_matvec), for the long
            rows of coarse Galerkin operators where a one-lane chain is latency-bound.
        Which family applies is a rule on the matrix; coarse_format='exact' keeps every
        operator in the exact family. fine_format='autotune' times the family's kernels on each
        operator once and keeps the fastest (self.tuning); any other value forces that format.
        first_level: the global index of self.levels[0] (a hierarchy that continues another one,
        e.g. the replicated tail of the distributed setup: the family rule uses the global
        level index)."""
        if coarse_format not in ("auto", "exact", "vector"):
            raise ValueError(f"coarse_format must be 'auto' or 'exact', got {coarse_format!r}")
        vec_min_row = self.VEC_MIN_MEAN_ROW if vec_min_row is None else vec_min_row
        self.tuning = []
        dev = torch.device("cuda", torch.cuda.current_device())
        flush = (torch.ones(autotune.FLUSH_BYTES // 8, dtype=torch.float64, device=dev)
                 if fine_format == "autotune" else None)
        for i, L in enumerate(self.levels):
            row = {}
            for name, M in (("A", L.A), ("P", L.P), ("R", L.R)):
                if fine_format != "autotune":
                    M.set_format(fine_format if fine_format != "vector" else "auto_exact")
                    row[name] = {"chosen": M.get_format()[:2]}
                    continue
                vector = (i + first_level > 0 and coarse_format != "exact"
                          and M.shape[0] <= (1 << 20) and M.nnz >= vec_min_row * M.shape[0])
                cands = autotune.candidates_for(M, "vector" if vector else "exact")

                def search(name=name, M=M, cands=cands):
                    x = torch.randn(M.shape[1], dtype=torch.float64, device=dev)
                    y = torch.zeros(M.shape[0], dtype=torch.float64, device=dev)
                    # This site's rules. Builds that would be refused are not tried (at C4 they
                    # were half the autotune, 0.46 of 0.99 s): a SELL, dictionary-SELL or sorted
                    # limit of one variant (too many column offsets or values, a row over a
                    # block) holds for the others, and block dictionaries (sorted/2) are refused
                    # when the <= 256-value table applies (known from sorted/0). A sigma-sorted
                    # variant only reorders rows by length: it does not close a large gap to the
                    # best format (C4 A_0: built in 0.18 s, it ran at 106 us, rowpat at 56).
                    chosen, us, pruned = autotune.search(
                        cands, {c: autotune.lower_bound_us(M, name, c[0]) for c in cands},
                        lambda fmt, arg: autotune.time_format(M, fmt, arg, x, y, kind=name,
                                                              flush=flush),
                        refuses_family=lambda fmt, arg: (fmt in ("sell_dict", "sell")
                                                         or (fmt, arg) == ("sorted", 0)),
                        sigma_skip=autotune.SIGMA_SKIP_RATIO,
                        value_dict=lambda: M.get_format()[1] == 1)
                    return {"chosen": chosen, "us": us, "pruned": pruned}
                row[name] = autotune.cached(
                    (name, M.shape, M.nnz, M.fingerprint(), tuple(cands)), search)
                fmt, arg = row[name]["chosen"].split("/")
                M.set_format(fmt, int(arg))
            self.tuning.append(row)
        self.attach_dinvs()

    def attach_dinvs(self):
        """Let every rowpat level operator take its Jacobi weights from its pattern table."""
        for L in self.levels:
            if L.A.get_format()[0] == "rowpat":
                L.A.attach_dinv(L.dinv)

    def set_factored_prolong(self, level=0, on=True):
        """Opt-in (VERDICT r04 Next #5): apply level `level`'s prolongation factored, x += t -
        (w / a_ii) (A t) with t = Agg e (P = (I - w D^-1 A) Agg, ns/lib/multigrid.py:102-108),
        through the level operator's uniform row-pair kernel (csrc/spmv.hip spmv_fadd) instead
        of streaming the explicit P. Same operator, different rounding: NOT bitwise the explicit
        P @ e (tests hold it to the oracle cycle at rtol 1e-11). Needs the level's aggregates
        (built here, not supplied as P) and a constant-stencil operator; raises MlamgError
        (EUNSUPPORTED) otherwise. on=False restores x += P e."""
        L = self.levels[level]
        if not on:
            call("mlamg_hier_set_factored_prolong", self.handle, int(level), None, None, None)
            self._factored.pop(level, None)
            return
        if self.recipe != "mlamg_sa" or not L.sa_prolong:
            # pyamg_sa's P = T - (w/rho) D^-1 A T smooths the normalised candidate T, not the
            # 0/1 aggregate operator: the factored form would be a different prolongator
            raise _lib.MlamgError(_lib.MLAMG_EUNSUPPORTED, "factored prolongation needs "
                                  "P = (I - w D^-1 A) Agg built by Hierarchy.build "
                                  f"(recipe {self.recipe!r}, level {level})")
        if L.agg_col is None or L.omega is None:
            raise ValueError("factored prolongation needs the level's aggregates and SA weight")
        ip, ij, ax = L.A.arrays()
        h = ctypes.c_void_p()
        n = L.A.shape[0]
        call("mlamg_csr_create", n, n, L.A.nnz, ctypes.c_void_p(ip), ctypes.c_void_p(ij),
             ctypes.c_void_p(ax), _lib.MLAMG_WRAP_DEVICE, ctypes.byref(h))
        A_uni = DeviceCSR(h, keep=(L.A,))  # wraps L.A's arrays: keep L.A alive
        A_uni.set_format("rowpat")
        c = L.A.diag_inv(L.omega)  # w / a_ii
        A_uni.attach_dinv(c)
        call("mlamg_hier_set_factored_prolong", self.handle, int(level), A_uni.handle,
             ptr(L.agg_col), ptr(c))
        self._factored[level] = (A_uni, c)

    def formats(self):
        return [{"A": L.A.get_format(), "P": L.P.get_format(), "R": L.R.get_format()}
                for L in self.levels]

    def set_formats(self, formats):
        """Apply a formats() list (e.g. rank 0's autotune result on every rank, so that the
        replicated hierarchies of a distributed run sum every row in the same order)."""
        if len(formats) != len(self.levels):
            raise ValueError("formats list does not match the number of levels")
        for L, f in zip(self.levels, formats):
            for name in ("A", "P", "R"):
                fmt, arg = f[name][0], f[name][1]
                getattr(L, name).set_format(fmt, int(arg))
        self.attach_dinvs()

    @classmethod
    def build(cls, A, *, alpha=0.1, strength_mode="invabs", aggregation="bellman_ford",
              max_coarse=1000, max_levels=10, jacobi_weight=2.0 / 3.0, seed=0, sort_seeds=True,
              lanczos_tol=1e-15, lanczos_iter=20000, lloyd_maxiter=10, nu_pre=1, nu_post=1,
              fine_format="autotune", coarse_format="auto", verbose=False, finalize=True,
              aggregates=None, prolongators=None, coarse_order="seed"):
        """Smoothed-aggregation hierarchy built on the GPU.

        Per level: strength -> seeds RandomState(seed).permutation(n)[:ceil(alpha n)] ->
        seeded Bellman-Ford (or Lloyd) aggregates -> SA prolongator P = (I - w D^-1 A) Agg with
        w = (4/3)/lambda_max(D^-1 A) (ns/lib/multigrid.py:102-108) -> A_c = P^T A P (:165).

        aggregation:
          'bellman_ford' (default): every level the order-independent seeded Bellman-Ford
              (label = smallest seed among tight predecessors), seeds sorted (sort_seeds);
          'reference': level 0 is the reference's "dumb" recipe of
              utils/evaluate_dataset.py:80-90 exactly — unsorted RandomState(seed) seeds, the
              in-place row-major push sweeps of ns/lib/graph.py:40-51 in fp32
              (mlamg_bellman_ford) and nearest_center_to_agg's columns (graph.py:56-86: column t
              = seeds[t]); coarser levels (no reference counterpart) as 'bellman_ford'.
              coarse_order='sorted' relabels the level-0 aggregates in ascending seed order
              (the same aggregates — each column is the same node set — permuted so coarse
              unknowns follow the fine ordering: locality, and the contiguous coarse ownership
              the distributed executor needs); 'seed' keeps the reference's column order;
          'lloyd': pyamg lloyd_cluster with the order-independent rule.

        aggregates / prolongators: supplied instead of computed, for the first levels — e.g. the
        learned aggregates of C5 or the learned P of the MLAMG PC
        (ns/preconditioner/MLAMG.py:105-121). Each is one item (level 0) or a list (levels
        0, 1, ...); an aggregate item is a label vector (node -> aggregate column, -1 = none)
        or an n x k 0/1 matrix (scipy or DeviceCSR), and is smoothed into P as above; a
        prolongator item is used as P as given (no smoothing). jacobi_weight="sa" smooths every
        level with its SA weight w instead of a fixed one."""
        if aggregation not in ("bellman_ford", "reference", "lloyd"):
            raise ValueError(f"unknown aggregation {aggregation!r}")
        if coarse_order not in ("seed", "sorted"):
            raise ValueError(f"coarse_order must be 'seed' or 'sorted', got {coarse_order!r}")
        from . import sa_setup
        H = cls()
        H.jacobi_weight = jacobi_weight
        H.aggregation = aggregation
        H.coarse_order = coarse_order
        t_all = time.perf_counter()
        tm = sa_setup.build_levels(
            H, as_device(A), alpha=alpha, strength_mode=strength_mode, aggregation=aggregation,
            max_coarse=max_coarse, max_levels=max_levels, jacobi_weight=jacobi_weight, seed=seed,
            sort_seeds=sort_seeds, lanczos_tol=lanczos_tol, lanczos_iter=lanczos_iter,
            lloyd_maxiter=lloyd_maxiter, fine_format=fine_format, verbose=verbose,
            aggregates=aggregates, prolongators=prolongators, coarse_order=coarse_order)
        if not finalize:  # setup only (e.g. to take P for a two-level cycle)
            return H
        t5 = time.perf_counter()
        H.apply_formats(fine_format, coarse_format)
        torch.cuda.synchronize()
        t6 = time.perf_counter()
        H._finalize(nu_pre, nu_post)
        torch.cuda.synchronize()
        tm["formats"] = t6 - t5
        tm["dense"] = time.perf_counter() - t6
        tm["total"] = time.perf_counter() - t_all
        H.timings = tm
        return H

    @classmethod
    def pyamg_sa(cls, A, *, max_levels=10, max_coarse=10, theta=0.0, omega=4.0 / 3.0,
                 improve_iterations=4, rho="lanczos", B=None, fine_format="csr_stream",
                 coarse_format="exact", verbose=False,
                 smoother=("block_gauss_seidel", {"sweep": "symmetric"}),
                 smoother_rho="arnoldi"):
        """pyamg.aggregation.smoothed_aggregation_solver(A, max_levels=max_levels) with pyamg's
        defaults — the multilevel solver of the reference's PyAMG preconditioner
        (ns/preconditioner/PyAMG.py:94) — built on the GPU. Per level, while n > max_coarse
        and fewer than max_levels levels:
          C = symmetric_strength_of_connection(A, theta)          mlamg_symmetric_strength
          AggOp = standard_aggregation(C)                          mlamg_standard_aggregation
          level 0: B <- 4 symmetric block Gauss-Seidel sweeps on A B = 0 from B = ones
                   (improve_candidates, level 0 only)              mlamg_gs_create_ex
          T, B_c = fit_candidates(AggOp, B)                        mlamg_fit_candidates
          P = T - (omega / rho) (D^-1 A) T  (jacobi_prolongation_smoother: D^-1 A by row
              scaling with get_diagonal(inv=True), scaled by omega / rho, times T, subtracted)
          R = P^T;  A_c = (R A) P
        Coarsest level: scipy.linalg.pinv(A_c) applied as a dense product (pyamg's 'pinv'
        coarse solver; the same scipy call). Smoother: symmetric block Gauss-Seidel, one
        iteration before and after the coarse correction (pyamg's presmoother/postsmoother).
        rho: rho(D^-1 A); 'lanczos' (default) the converged device Lanczos value, 'arnoldi'
        pyamg's approximate_spectral_radius estimate (15-step Arnoldi from np.random.rand: draws
        from numpy's global generator, as pyamg does), or a number / per-level list.
        pyamg is absent here: parity unpinned; every setup kernel is bitwise the oracle's
        restatement (oracle/oracle.c pyamg_*). Summation orders of pyamg's BSR products are not
        restated (the Galerkin product sums over k ascending, as scipy's CSR/CSC kernels do).
        smoother=('chebyshev', {'degree': 3, 'iterations': 1, 'lower_bound': 1/30,
        'upper_bound': 1.1}) (or the bare name) smooths every level with pyamg's polynomial
        smoother instead (presmoother = postsmoother = that pair; smoothing.setup_chebyshev):
        per level the coefficients for rho(A) = smoother_rho — 'arnoldi' (default) pyamg's
        approximate_spectral_radius(A), which draws from numpy's global generator, or a number /
        per-level list. improve_candidates stays Gauss-Seidel."""
        from . import pyamg_setup
        sm_name, sm_opts = _smoother_spec(smoother)
        if sm_name == "chebyshev":
            sm_opts = _chebyshev_options(sm_opts)
        elif sm_name != "block_gauss_seidel" or sm_opts not in ({}, {"sweep": "symmetric"}):
            raise NotImplementedError("smoother must be pyamg's default symmetric "
                                      f"block_gauss_seidel or 'chebyshev', got {smoother!r}")
        if max_levels < 1:
            raise ValueError("max_levels must be >= 1")
        H = cls()
        H.recipe = "pyamg_sa"
        H.jacobi_weight = None
        t_all = time.perf_counter()
        tm = pyamg_setup.build_levels(
            H, as_device(A), B, max_levels=max_levels, max_coarse=max_coarse, theta=theta,
            omega=omega, improve_iterations=improve_iterations, rho=rho, verbose=verbose)
        t7 = time.perf_counter()
        if H.levels:
            H.apply_formats(fine_format, coarse_format)
        t8 = time.perf_counter()
        H._finalize_pinv(gauss_seidel=sm_name != "chebyshev")
        if sm_name == "chebyshev":
            H._set_chebyshev(sm_opts, smoother_rho)
        torch.cuda.synchronize()
        tm["formats"] = t8 - t7
        tm["coarse_and_smoothers"] = time.perf_counter() - t8
        tm["total"] = time.perf_counter() - t_all
        H.timings = tm
        return H

    def _finalize_pinv(self, gauss_seidel=True):
        """pyamg's default coarse solver ('pinv': scipy.linalg.pinv of the dense A_c, applied as
        a product) and symmetric block Gauss-Seidel V(1,1) smoothing on every level
        (gauss_seidel=False: the caller sets another smoother)."""
        import scipy.linalg
        from .multigrid import GaussSeidel
        Ad = self.Ac.to_scipy().toarray()
        Pinv = np.ascontiguousarray(scipy.linalg.pinv(Ad), dtype=np.float64)
        self.coarse_pinv = Pinv
        h = ctypes.c_void_p()
        call("mlamg_dense_create_matrix", Pinv.ctypes.data_as(ctypes.c_void_p),
             int(Pinv.shape[0]), ctypes.byref(h), stream_ptr())
        self.dense = h
        self._assemble(1, 1)
        if not gauss_seidel:
            return
        for i, L in enumerate(self.levels):
            if L.gs is None:
                L.gs = GaussSeidel(L.A, "symmetric", block=True)
            call("mlamg_hier_set_level_smoother", self.handle, i, L.gs.handle)

    def _set_chebyshev(self, opts, rho):
        """Make the recipe's smoother pyamg's Chebyshev polynomial (setup_chebyshev per level)."""
        from .multigrid import chebyshev_coefficients
        from .pyamg_setup import level_rho
        from .strength import approximate_spectral_radius
        o = _chebyshev_options(opts)
        coeffs = []
        for lvl, L in enumerate(self.levels):
            L.rho_A = float(level_rho(
                rho, lvl, {"arnoldi": lambda: approximate_spectral_radius(L.A)}, "smoother_rho"))
            coeffs.append(chebyshev_coefficients(L.rho_A, int(o["degree"]),
                                                 float(o["lower_bound"]),
                                                 float(o["upper_bound"])))
        self._recipe_poly = (coeffs, int(o["iterations"]))
        self.set_polynomial_smoother(coeffs, int(o["iterations"]))

    def set_polynomial_smoother(self, coefficients, iterations=1):
        """Smooth with pyamg's relaxation.polynomial (multigrid.Polynomial) on every level of a
        finalised hierarchy, whatever built it: each of the cycle's nu_pre / nu_post sweeps is
        `iterations` iterations with `coefficients` (highest power first, no constant term;
        multigrid.chebyshev_coefficients makes pyamg's) — one sequence for all levels or a list
        of one sequence per level. Both cycle() and cycle_multi() take such levels, bitwise per
        column. None removes them and restores the smoother the recipe set up (weighted Jacobi,
        Gauss-Seidel, or pyamg_sa(smoother='chebyshev')'s own polynomials), bitwise. Returns
        self."""
        from .multigrid import Polynomial
        if self.handle is None:
            raise ValueError("the hierarchy is not finalised")
        if coefficients is None:
            if self._recipe_poly is not None:
                return self.set_polynomial_smoother(*self._recipe_poly)
            for i, L in enumerate(self.levels):
                call("mlamg_hier_set_level_polynomial", self.handle, i, None, 1)
                if L.gs is not None and self.recipe_gs(i):
                    call("mlamg_hier_set_level_smoother", self.handle, i, L.gs.handle)
                L.poly = None
            self.poly_iterations = 1
            return self
        per_level = (isinstance(coefficients, (list, tuple)) and len(coefficients) > 0
                     and np.ndim(coefficients[0]) == 1)
        if per_level and len(coefficients) != len(self.levels):
            raise ValueError(f"{len(coefficients)} coefficient sets for {len(self.levels)} levels")
        if int(iterations) < 1:
            raise ValueError("iterations must be >= 1")
        new = [Polynomial(L.A, coefficients[i] if per_level else coefficients)
               for i, L in enumerate(self.levels)]
        for i, (L, S) in enumerate(zip(self.levels, new)):
            call("mlamg_hier_set_level_polynomial", self.handle, i, S.handle, int(iterations))
            L.poly = S  # the handle a level had is released only now
        self.poly_iterations = int(iterations)
        return self

    def recipe_gs(self, level):
        """Whether the recipe smooths `level` with its Gauss-Seidel handle (pyamg_sa keeps one
        on level 0 for the candidate improvement even when it smooths with Chebyshev)."""
        return self._recipe_poly is None and self.levels[level].gs is not None

    # coarsest solve: a dense inverse up to this many rows (its setup is O(n_c^3)), above it
    # PCG preconditioned by an inner hierarchy of the coarse operator (csrc/pcg.hip)
    DENSE_MAX = 4096
    # the reference's two-level solve factors A_H once for ~30 cycles: there the O(n_c^3) dense
    # factor (device-wide, fp64 matrix cores) beats a PCG solve per cycle up to larger n_c
    TWO_LEVEL_DENSE_MAX = 10240
    COARSE_RTOL = 1e-12
    # the PCG preconditioner's hierarchy stops coarsening at this size (its coarsest operator is
    # then solved by the dense inverse)
    PCG_INNER_MAX_COARSE = 4096
    PCG_INNER_NU = 2  # V(nu, nu) preconditioner cycle (symmetric for any nu)

    # the dense solver's size limit (dense.hip mlamg_dense_create): an operator PCG may not take
    # (not symmetric) still gets an exact inverse up to this size
    DENSE_LIMIT = 32768
    SYMMETRY_RTOL = 1e-12  # dense.hip's "symmetric to rounding" test

    # coarsest solve of an operator that is not SPD and beyond DENSE_LIMIT rows: restarted GMRES
    # (restart GMRES_RESTART, at most GMRES_MAXITER restart cycles) preconditioned by one V-cycle
    # of an inner hierarchy, to ||r|| <= GMRES_RTOL ||b||; a solve whose final relative residual
    # stays above GMRES_FAIL_RTOL is a failed coarse solve (CoarseSolveError, like a SuperLU
    # factorisation failure)
    GMRES_RTOL = 1e-14
    GMRES_RESTART = 50
    GMRES_MAXITER = 20
    GMRES_FAIL_RTOL = 1e-10

    def _finalize(self, nu_pre, nu_post, dense_max=None, coarse_rtol=None, coarse=None):
        """coarse: None chooses (dense inverse up to dense_max rows; above, PCG for a symmetric
        A_c, else the dense inverse up to DENSE_LIMIT rows, else GMRES); 'gmres' forces GMRES."""
        dense_max = self.DENSE_MAX if dense_max is None else dense_max
        n_c = self.Ac.shape[0]
        use_gmres = coarse == "gmres"
        if not use_gmres and n_c > dense_max and not csr_symmetric(self.Ac, self.SYMMETRY_RTOL):
            # PCG needs an SPD A_c (a Galerkin P^T A P of an SPD A is symmetric to rounding);
            # SuperLU, which the reference uses, takes any nonsingular A_H: an exact dense
            # inverse up to DENSE_LIMIT rows, GMRES beyond
            if n_c > self.DENSE_LIMIT:
                use_gmres = True
            else:
                dense_max = n_c
        if use_gmres:
            self._make_coarse_gmres()
        elif n_c <= dense_max:
            h = ctypes.c_void_p()
            call("mlamg_dense_create", self.Ac.handle, ctypes.byref(h), stream_ptr())
            self.dense = h
        else:
            self._make_coarse_pcg(self.COARSE_RTOL if coarse_rtol is None else coarse_rtol)
        self._assemble(nu_pre, nu_post)

    def _assemble(self, nu_pre, nu_post):
        """Create the mlamg_hier handle: the levels, the coarse solver this hierarchy holds (a
        dense inverse or pinv matrix, PCG, or GMRES with its four parameters) and the smoothing
        counts."""
        self.nu_pre, self.nu_post = nu_pre, nu_post
        hh = ctypes.c_void_p()
        call("mlamg_hier_create", ctypes.byref(hh))
        self.handle = hh
        for L in self.levels:
            call("mlamg_hier_add_level", hh, L.A.handle, ptr(L.dinv), L.P.handle, L.R.handle)
        if self.dense is not None:
            call("mlamg_hier_set_coarse", hh, self.Ac.handle, self.dense)
        elif self.pcg is not None:
            call("mlamg_hier_set_coarse_pcg", hh, self.Ac.handle, self.pcg)
        else:
            call("mlamg_hier_set_coarse_gmres", hh, self.Ac.handle, self.inner.handle,
                 float(self.GMRES_RTOL), float(self.GMRES_FAIL_RTOL), int(self.GMRES_RESTART),
                 int(self.GMRES_MAXITER))
        call("mlamg_hier_set_smoothing", hh, int(nu_pre), int(nu_post))

    def _make_coarse_gmres(self):
        """Coarsest solve for a coarse operator that is not SPD (non-symmetric, or indefinite:
        PCG broke down) and too large for the dense inverse: GMRES on A_c preconditioned by one
        V(2,2) cycle of an inner smoothed-aggregation hierarchy of A_c (weighted Jacobi w = 2/3,
        a dense coarsest inverse) — the reference factors any nonsingular A_H with SuperLU
        (ns/lib/multigrid.py:165-170)."""
        self.inner = Hierarchy.build(self.Ac, alpha=0.1, max_coarse=self.PCG_INNER_MAX_COARSE,
                                     jacobi_weight=2.0 / 3.0, lanczos_tol=1e-8,
                                     nu_pre=self.PCG_INNER_NU, nu_post=self.PCG_INNER_NU,
                                     fine_format="csr_stream", coarse_format="exact")
        self.coarse_gmres = True

    def _make_coarse_pcg(self, rtol, maxit=200):
        """Coarsest solve for an operator too large for the dense inverse (the reference
        factorises any size with SuperLU, ns/lib/multigrid.py:168): PCG on A_c with one V-cycle
        of an inner smoothed-aggregation hierarchy of A_c as preconditioner, to
        ||r|| <= rtol ||b||. The inner hierarchy smooths with the per-level SA weight
        w = (4/3)/lambda_max(D^-1 A) (w * lambda_max < 2: a convergent, symmetric V-cycle, i.e.
        an SPD preconditioner for an SPD A_c)."""
        self.inner = Hierarchy.build(self.Ac, alpha=0.1, max_coarse=self.PCG_INNER_MAX_COARSE,
                                     jacobi_weight="sa", lanczos_tol=1e-8,
                                     nu_pre=self.PCG_INNER_NU,
                                     nu_post=self.PCG_INNER_NU,
                                     fine_format="csr_stream", coarse_format="exact")
        h = ctypes.c_void_p()
        call("mlamg_pcg_create", self.Ac.handle, self.inner.handle, float(rtol), int(maxit),
             ctypes.byref(h))
        self.pcg = h

    def coarse_stats(self):
        """PCG / GMRES coarse solver statistics (None with a dense coarse inverse): iterations
        of the last solve, solves that stopped at maxit, total iterations, largest final
        relative residual (GMRES: also the number of solves)."""
        if getattr(self, "coarse_gmres", False) and self.handle:
            sv, a, c, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
            d = ctypes.c_double()
            call("mlamg_hier_coarse_gmres_stats", self.handle, ctypes.byref(sv), ctypes.byref(a),
                 ctypes.byref(c), ctypes.byref(b), ctypes.byref(d))
            return {"solver": "gmres", "solves": sv.value, "last_iters": a.value,
                    "not_converged": b.value, "total_iters": c.value,
                    "max_rel_residual": d.value, "breakdowns": 0}
        if getattr(self, "pcg", None) is None:
            return None
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        d = ctypes.c_double()
        e = ctypes.c_int32()
        call("mlamg_pcg_stats", self.pcg, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
             ctypes.byref(d), stream_ptr())
        call("mlamg_pcg_breakdowns", self.pcg, ctypes.byref(e), stream_ptr())
        return {"last_iters": a.value, "not_converged": b.value, "total_iters": c.value,
                "max_rel_residual": d.value, "breakdowns": e.value}

    def check_coarse(self):
        """Raise if a PCG coarse solve broke down (A_c or its preconditioner not positive
        definite: the iterate is not a solve of the coarse system). Syncs."""
        if self.pcg is None and not self.coarse_gmres:
            return
        st = self.coarse_stats()
        if st.get("solver") == "gmres":  # a failed solve already ended its call (_gmres_call)
            return
        if st is not None and st["breakdowns"] > self._breakdowns_seen:
            self._breakdowns_seen = st["breakdowns"]
            raise CoarseSolveError(f"PCG coarse solve broke down ({st['breakdowns']} solves): "
                                   "the coarse operator is not positive definite")

    # ------------------------------------------------------------------ cycling
    def _solve_call(self, fn, *args):
        """A C-ABI call that runs this hierarchy's cycles: a GMRES coarse solve that did not
        converge ends it with EINVAL ("did not converge") -> CoarseSolveError (the reference's
        factorisation failure, ns/lib/multigrid.py:167-170)."""
        try:
            return call(fn, *args)
        except MlamgError as e:
            if self.coarse_gmres and "did not converge" in str(e):
                raise CoarseSolveError(str(e)) from None
            raise

    def cycle(self, b, x, n_cycles, tol=None, use_graph=True, history=True):
        """Run up to n_cycles V-cycles in place on x (device tensors). Returns the residual
        history ||b - A x||_2 after each cycle (numpy, truncated at convergence). tol=None runs
        every cycle; a number (0 included) stops after the first cycle whose norm is <= tol."""
        dev = x.device
        hist = torch.zeros(max(n_cycles, 1), dtype=torch.float64, device=dev) if history else None
        done = ctypes.c_int32()
        self._solve_call("mlamg_hier_vcycle", self.handle, ptr(rhs_arg(b)), ptr(x),
                         int(n_cycles), _tol_arg(tol), ptr(hist), ctypes.byref(done),
                         int(bool(use_graph)), stream_ptr())
        self.check_coarse()
        if not history:
            return None
        return hist[: int(done.value)].cpu().numpy()

    def cycle_async(self, b, x, n_cycles, use_graph=True, zero_rhs=None):
        """Launch n_cycles V-cycles without reading anything back (for timing). zero_rhs: None
        = detect an all-zero b (rhs_arg: one reduction and a sync), True / False = as given
        (False streams b even when it is zero: the general-b kernels)."""
        if zero_rhs is None:
            bb = rhs_arg(b)
        else:
            bb = None if zero_rhs else b
            if zero_rhs and b is not None and bool(torch.count_nonzero(b.view(torch.int64))):
                raise ValueError("zero_rhs=True with a nonzero b")
        self._solve_call("mlamg_hier_vcycle", self.handle, ptr(bb), ptr(x), int(n_cycles),
                         _tol_arg(None), None, None, int(bool(use_graph)), stream_ptr())

    def solve(self, b, x0=None, tol=1e-8, maxiter=500, return_history=False):
        """Stationary V-cycle iteration until ||b - A x||_2 <= tol (absolute, MLAMG.py:194);
        tol=None runs all maxiter cycles."""
        _, bd, xd = self._krylov_in(b, x0)
        hist = self.cycle(bd, xd, maxiter, tol=tol)
        x = xd.cpu().numpy() if not isinstance(b, torch.Tensor) else xd
        return (x, hist) if return_history else x

    def _krylov_in(self, b, x0, in_place=False):
        """(A, b on the device, the iterate: a copy of x0, or zeros) for a solver wrapper;
        in_place takes a cuda fp64 b as it is (e.g. a column slice of a wider tensor)."""
        A = self.levels[0].A if self.levels else self.Ac
        if in_place and isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.float64:
            bd = b
        else:
            bd = to_device_vec(b)
        if x0 is None:
            xd = torch.zeros(tuple(bd.shape), dtype=torch.float64, device=bd.device)
        else:
            xd = to_device_vec(x0).clone()
        return A, bd, xd

    def _krylov_out(self, b, xd):
        """The iterate as a GMRES wrapper returns it (numpy for a numpy b, the tensor for a
        tensor b), after the check for a coarse solve that broke down in the preconditioner."""
        self.check_coarse()
        return xd if isinstance(b, torch.Tensor) else xd.cpu().numpy()

    def gmres(self, b, x0=None, rtol=1e-5, restart=20, maxiter=None, return_info=False):
        """GMRES on A x = b preconditioned by one V-cycle of this hierarchy (mlamg_gmres:
        scipy.sparse.linalg.gmres's algorithm — left-preconditioned, restarted MGS — with
        ||b - A x|| <= rtol ||b||; the Krylov acceleration of ns/preconditioner/PyAMG.py:119).
        x0=None starts from 0. Returns x (numpy in -> numpy out, tensor in -> tensor out), plus
        {"info", "inner_iters", "presid"} (presid: preconditioned residual estimate / ||b|| per
        Krylov step) with return_info=True. A 2-D b is a block of right-hand sides:
        gmres_multi(b, x0, ...)."""
        if getattr(b, "ndim", 1) == 2:
            return self.gmres_multi(b, x0, rtol=rtol, restart=restart, maxiter=maxiter,
                                    return_info=return_info)
        A, bd, xd = self._krylov_in(b, x0)
        cap = 4096
        hist = (ctypes.c_double * cap)()
        info, inner = ctypes.c_int(), ctypes.c_int()
        self._solve_call("mlamg_gmres", A.handle, self.handle, ptr(bd), ptr(xd), float(rtol),
                         int(restart), int(maxiter or 0), int(x0 is None), ctypes.byref(info),
                         ctypes.byref(inner), hist, cap, stream_ptr())
        x = self._krylov_out(b, xd)
        if not return_info:
            return x
        k = min(inner.value, cap)
        return x, {"info": info.value, "inner_iters": inner.value,
                   "presid": np.array(hist[:k])}

    def gmres_multi(self, B, X0=None, rtol=1e-5, restart=20, maxiter=None, return_info=False):
        """gmres on the (n, k) block B of k <= 64 right-hand sides at once (mlamg_gmres_mv): the
        columns run in lock-step, so every Krylov step applies the operator, the preconditioner
        (one block cycle) and each Gram-Schmidt reduction once for all k columns. Column j of the
        result, and its entries of the info, are bitwise gmres(B[:, j], X0[:, j], ...): each
        column stops on its own ||b_j - A x_j|| <= rtol ||b_j|| and is frozen from then on.
        X0=None starts from 0. B (and X0) may be column slices of wider tensors. Returns X (numpy
        in -> numpy out, tensor in -> tensor out), plus {"info": (k,), "inner_iters": (k,),
        "presid": list of k arrays} with return_info=True. The preconditioner is the block
        cycle, with cycle_multi's coarse solves and refusals: Gauss-Seidel levels need
        enable_block_gauss_seidel() first, 'vector'-format operators enable_block_vector()."""
        from .sparse import mv_block
        A, Bd, Xd = self._krylov_in(B, X0, in_place=True)
        n = A.shape[0]
        k, ldb = mv_block(Bd, n, "B")
        if tuple(Xd.shape) != (n, k):
            raise ValueError(f"X0 has shape {tuple(Xd.shape)}, expected {(n, k)}")
        cap = 4096
        hist = np.zeros((cap, k), dtype=np.float64)
        info = np.zeros(k, dtype=np.int32)
        inner = np.zeros(k, dtype=np.int32)
        P_i32 = ctypes.POINTER(ctypes.c_int32)
        self._solve_call("mlamg_gmres_mv", A.handle, self.handle, ptr(Bd), ldb, ptr(Xd), k, k,
                         float(rtol), int(restart), int(maxiter or 0), int(X0 is None),
                         info.ctypes.data_as(P_i32), inner.ctypes.data_as(P_i32),
                         hist.ctypes.data, cap, stream_ptr())
        X = self._krylov_out(B, Xd)
        if not return_info:
            return X
        return X, {"info": info, "inner_iters": inner,
                   "presid": [hist[: min(int(inner[j]), cap), j].copy() for j in range(k)]}

    def gmres_householder(self, b, x0=None, tol=1e-5, maxiter=None, return_info=False):
        """pyamg.krylov.gmres(A, b, x0, tol, maxiter, M=one V-cycle) with its default
        Householder orthogonalisation (mlamg_gmres_householder): what pyamg's
        MultilevelSolver.solve(b, tol, accel='gmres') runs (ns/preconditioner/PyAMG.py:119).
        Returns x (numpy in -> numpy out, tensor in -> tensor out), plus {"info", "iters",
        "residuals"} (preconditioned residual norms: initial, per step, final) with
        return_info=True."""
        A, bd, xd = self._krylov_in(b, x0)
        cap = 4096
        hist = (ctypes.c_double * cap)()
        info, iters = ctypes.c_int(), ctypes.c_int()
        self._solve_call("mlamg_gmres_householder", A.handle, self.handle, ptr(bd), ptr(xd),
                         float(tol), int(maxiter or 0), int(x0 is None), ctypes.byref(info),
                         ctypes.byref(iters), hist, cap, stream_ptr())
        x = self._krylov_out(b, xd)
        if not return_info:
            return x
        # recorded: the initial norm, one per step except the last (the budget's last step, or
        # the step whose estimate met tol: pyamg breaks before appending it), the final norm
        it = iters.value
        k = min(1 if it == 0 else it + 1, cap)
        return x, {"info": info.value, "iters": it, "residuals": np.array(hist[:k])}

    def enable_block_gauss_seidel(self, on=True):
        """Let cycle_multi / precondition(B) take this hierarchy's Gauss-Seidel levels
        (mlamg_hier_set_mv_gauss_seidel): each such level smooths the whole block with one block
        sweep (mlamg_gs_sweep_mv), and column j keeps the bits of the single-vector cycle on
        column j. Off by default, where a Gauss-Seidel level is refused. Returns self."""
        call("mlamg_hier_set_mv_gauss_seidel", self.handle, int(bool(on)))
        return self

    def enable_block_vector(self, on=True):
        """Let cycle_multi / precondition(B) take this hierarchy's operators in the 'vector'
        format (mlamg_hier_set_mv_vector), where build()'s default coarse_format='auto' puts
        every long-row coarse operator: each launch of the block cycle then follows its own
        operator's format — the canonical-order kernel (mlamg_spmm_vec and its kin) for a
        'vector' operator, the scipy-order one for the rest — and column j keeps the bits of the
        single-vector cycle on column j. Off by default, where such an operator is refused.
        Returns self."""
        call("mlamg_hier_set_mv_vector", self.handle, int(bool(on)))
        return self

    def cycle_multi(self, B, X, n_cycles, norm="residual", remove_mean=False, history=True):
        """Run n_cycles V-cycles in place on the block X of k <= 64 vectors (cuda fp64 (n, k)
        tensors with unit column stride; B=None: a zero right-hand side) through the
        multi-vector kernels (mlamg_hier_vcycle_mv): every operator is streamed once for all k
        columns, and column j has the bits of the single-vector cycle on column j.
        remove_mean subtracts each column's mean after every cycle's post-smoothing
        (ns/model/loss.py:89). Returns the (n_cycles, k) history (numpy) of ||b - A x||_2
        (norm='residual') or ||x||_2 (norm='x') per column, taken after the mean removal; None
        with history=False. A fixed cycle count, run eagerly. Weighted-Jacobi levels with a
        dense or a PCG coarse solve (the block PCG, mlamg_pcg_solve_mv: per column the bits and
        the iteration count of the single solve; a breakdown raises CoarseSolveError as in
        cycle()). Gauss-Seidel levels (two_level(smoother="gauss_seidel"), pyamg_sa) are taken
        after enable_block_gauss_seidel(), through the block sweep mlamg_gs_sweep_mv, and may mix
        with Jacobi levels. Operators in the 'vector' format (build()'s coarse_format='auto'
        puts the long-row coarse operators there) are taken after enable_block_vector(), through
        the canonical-order kernel mlamg_spmm_vec, and may mix with the other formats. Without
        the respective switch such a level or operator is refused, as are a GMRES coarse solve
        and a factored prolongation (MlamgError EUNSUPPORTED)."""
        from .sparse import mv_block
        if norm not in ("residual", "x"):
            raise ValueError(f"unknown norm {norm!r}")
        n = self.levels[0].A.shape[0] if self.levels else self.Ac.shape[0]
        k, ldx = mv_block(X, n, "X")
        ldb = 0
        if B is not None:
            kb, ldb = mv_block(B, n, "B")
            if kb != k:
                raise ValueError(f"B has {kb} columns, X has {k}")
        hist = (torch.zeros((max(n_cycles, 1), k), dtype=torch.float64, device=X.device)
                if history else None)
        self._solve_call("mlamg_hier_vcycle_mv", self.handle, ptr(B), ldb, ptr(X), ldx, k,
                         int(n_cycles), 0 if norm == "residual" else 1, int(bool(remove_mean)),
                         ptr(hist), stream_ptr())
        self.check_coarse()
        if not history:
            return None
        return hist[: int(n_cycles)].cpu().numpy()

    def precondition(self, b):
        """One V-cycle from a zero guess: the action of the preconditioner on b (a vector, or
        an (n, k) block of k <= 64 right-hand sides: one block cycle, column j bitwise
        precondition(b[:, j]); cycle_multi's coarse solves and refusals: a hierarchy with
        Gauss-Seidel levels, pyamg_sa's for one, needs enable_block_gauss_seidel() first, one
        with 'vector'-format operators, build()'s default on long-row coarse levels,
        enable_block_vector())."""
        _, bd, xd = self._krylov_in(b, None)
        (self.cycle_multi if getattr(b, "ndim", 1) == 2 else self.cycle)(bd, xd, 1, history=False)
        return xd if isinstance(b, torch.Tensor) else xd.cpu().numpy()

    def cycle_bytes(self, stored=False):
        """Bytes of one V-cycle. stored=False: operators priced as CSR (a
        CSR-equivalent figure); stored=True: priced as stored (the cycle's HBM roofline bytes)."""
        v = ctypes.c_double()
        call("mlamg_hier_cycle_format_bytes" if stored else "mlamg_hier_cycle_bytes",
             self.handle, ctypes.byref(v))
        return float(v.value)

    # ------------------------------------------------------------------ info
    @property
    def n_levels(self):
        return len(self.levels) + 1

    def operator_complexity(self):
        nnz = sum(L.A.nnz for L in self.levels) + self.Ac.nnz
        return nnz / self.levels[0].A.nnz if self.levels else 1.0

    def describe(self):
        rows = []
        for i, L in enumerate(self.levels):
            if L.poly is not None:
                sm = (f"polynomial (degree {L.poly.coefficients.size}, "
                      f"{self.poly_iterations} iteration(s) per sweep)")
            elif L.gs is not None and self.recipe_gs(i):
                sm = (("block " if L.gs.block else "") + f"gauss_seidel ({L.gs.sweep_dir})")
            else:
                sm = "weighted jacobi"
            rows.append({"level": i, "n": L.A.shape[0], "nnz": L.A.nnz,
                         "P_nnz": L.P.nnz, "omega": L.omega, "lambda_max": L.lam,
                         "lanczos_iters": L.lanczos_iters, "bf_sweeps": L.bf_sweeps,
                         "smoother": sm})
        rows.append({"level": len(self.levels), "n": self.Ac.shape[0], "nnz": self.Ac.nnz,
                     "coarse": "dense inverse" if self.dense is not None
                     else ("GMRES, inner SA hierarchy" if self.coarse_gmres
                           else "PCG, inner SA hierarchy")})
        return rows

    def __del__(self):
        for attr, fn in (("handle", "mlamg_hier_destroy"), ("dense", "mlamg_dense_destroy"),
                         ("pcg", "mlamg_pcg_destroy")):
            h = getattr(self, attr, None)
            if h:
                try:
                    getattr(_lib.lib, fn)(h)
                except Exception:
                    pass
                setattr(self, attr, None)
