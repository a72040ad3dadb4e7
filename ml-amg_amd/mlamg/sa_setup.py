"""The levels of Hierarchy.build: the reference's aggregation-based SA recipe on the device, per
level from the strength graph through the Galerkin product (the recipe is described in
mlamg/hierarchy.py's module text and in Hierarchy.build)."""
import ctypes
import math
import time

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import call
from .graph import (aggregate_op_device, bellman_ford_device, labels_to_columns,
                    legacy_permutation, lloyd_cluster_device, modified_bellman_ford_device)
from .hierarchy import Level, _level_item, strength
from .multigrid import lambda_max_dinv_a
from .sparse import DeviceCSR, _device, as_device, csr_out, galerkin

_PHASES = ("count", "alloc", "expand", "sort", "runsum", "emit", "finalize", "free")


def _setup_phases(reset=False):
    """Accumulated SpGEMM phase wall times (ms) since the last reset (mlamg_setup_phase_times)."""
    buf = (ctypes.c_double * len(_PHASES))()
    call("mlamg_setup_phase_times", buf, len(_PHASES), int(bool(reset)))
    return {k: round(float(v), 2) for k, v in zip(_PHASES, buf)}


def _aggregate_operator(agg, n):
    """Agg (n x k, ones) on the device from a label vector (-1 = unaggregated) or a matrix."""
    if isinstance(agg, DeviceCSR):
        return agg
    if sp.issparse(agg):
        if agg.shape[0] != n:
            raise ValueError(f"aggregate matrix has {agg.shape[0]} rows, the operator {n}")
        A = sp.csr_matrix(agg, dtype=np.float64)
        A.data[:] = 1.0
        return DeviceCSR.from_scipy(A)
    lab = np.asarray(agg.cpu().numpy() if isinstance(agg, torch.Tensor) else agg).astype(np.int64)
    if lab.shape != (n,):
        raise ValueError(f"aggregate labels must have shape ({n},), got {lab.shape}")
    k = int(lab.max()) + 1 if lab.size else 0
    return aggregate_op_device(torch.as_tensor(lab.astype(np.int32)).to(_device()), k)


def build_levels(H, A_dev, *, alpha, strength_mode, aggregation, max_coarse, max_levels,
                 jacobi_weight, seed, sort_seeds, lanczos_tol, lanczos_iter, lloyd_maxiter,
                 fine_format, verbose, aggregates, prolongators, coarse_order):
    """Append Hierarchy.build's levels of A_dev to H (its keywords, as given there) and set
    H.Ac, H.galerkin_s and H.spgemm_phases_ms. Returns the seconds spent per setup phase."""
    tm = {"aggregation": 0.0, "lambda_max": 0.0, "prolongator": 0.0, "galerkin": 0.0}
    _setup_phases(reset=True)
    H.galerkin_s = []
    while True:
        n = A_dev.shape[0]
        if n <= max_coarse or len(H.levels) + 1 >= max_levels:
            break
        L = Level(A_dev)
        lvl = len(H.levels)
        P_given = _level_item(prolongators, lvl)
        Agg_given = _level_item(aggregates, lvl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if P_given is None and Agg_given is None:
            C = strength(A_dev, strength_mode)
            k = int(math.ceil(alpha * n))
            if isinstance(seed, (int, np.integer)) and 0 <= int(seed) < 2 ** 32:
                # RandomState(seed).permutation(n)[:k], bit for bit (device, csrc/seeds.hip)
                seeds = legacy_permutation(seed, n, k).cpu().numpy().astype(np.int64)
            else:  # a seed numpy takes otherwise (None, an array, a generator's state)
                seeds = np.random.RandomState(seed).permutation(n)[:k]
            if aggregation == "reference" and lvl == 0:
                # evaluate_dataset.py:80-90: push-order sweeps from the unsorted seeds
                seeds_dev = torch.as_tensor(seeds.astype(np.int32)).to(_device())
                _, lab, L.bf_sweeps = modified_bellman_ford_device(C, seeds_dev)
                if coarse_order == "sorted":
                    seeds = np.sort(seeds)
                    seeds_dev = torch.as_tensor(seeds.astype(np.int32)).to(_device())
                col = labels_to_columns(lab, seeds_dev)
                L.labels = lab
            else:
                if sort_seeds:
                    seeds = np.sort(seeds)
                seeds_dev = torch.as_tensor(seeds.astype(np.int32)).to(_device())
                if aggregation == "lloyd":
                    _, col, _, L.bf_sweeps = lloyd_cluster_device(C, seeds_dev,
                                                                  lloyd_maxiter, exact=False)
                else:
                    _, lab, L.bf_sweeps = bellman_ford_device(C, seeds_dev)
                    col = labels_to_columns(lab, seeds_dev)
                    L.labels = lab
            L.seeds = seeds
            L.Agg = aggregate_op_device(col, k)
            L.agg_col = col
            L.n_seeds = k
            del C
        elif P_given is None:
            L.Agg = _aggregate_operator(Agg_given, n)
            L.n_seeds = L.Agg.shape[1]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if P_given is None or jacobi_weight == "sa":
            if lvl == 0 and fine_format in ("autotune", "rowpat"):
                # Lanczos runs on the operator's own SpMV: a constant stencil gets its
                # row-pair format now (the autotune below reuses or replaces it)
                try:
                    A_dev.set_format("rowpat")
                except _lib.MlamgError as e:
                    if e.code != _lib.MLAMG_EUNSUPPORTED:
                        raise
            L.lam, L.lanczos_iters = lambda_max_dinv_a(A_dev, max_iter=lanczos_iter,
                                                       tol=lanczos_tol)
            L.omega = (4.0 / 3.0) / abs(L.lam)
        t2 = time.perf_counter()
        if P_given is None:
            S = csr_out("mlamg_sa_smoother", A_dev.handle, float(L.omega))
            L.P = S @ L.Agg
            L.sa_prolong = True
            del S
        else:
            L.P = as_device(P_given)
            if L.P.shape[0] != n:
                raise ValueError(f"level {lvl}: prolongator has {L.P.shape[0]} rows, "
                                 f"the operator {n}")
        if L.P.shape[1] >= n:
            raise ValueError(f"level {lvl}: P has {L.P.shape[1]} columns for {n} rows "
                             "(no coarsening)")
        L.R = L.P.transpose()
        L.dinv = A_dev.diag_inv(L.omega if jacobi_weight == "sa" else jacobi_weight)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        A_next = galerkin(L.R, A_dev, L.P)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        tm["aggregation"] += t1 - t0
        tm["lambda_max"] += t2 - t1
        tm["prolongator"] += t3 - t2
        tm["galerkin"] += t4 - t3
        H.galerkin_s.append(round(t4 - t3, 4))
        H.levels.append(L)
        if verbose:
            print(f"[mlamg] level {len(H.levels) - 1}: n={n} nnz={A_dev.nnz} "
                  f"seeds={L.n_seeds} bf_sweeps={L.bf_sweeps} lam={L.lam} "
                  f"({L.lanczos_iters} it) "
                  f"P nnz={L.P.nnz} -> n_c={A_next.shape[0]} nnz_c={A_next.nnz} "
                  f"[agg {t1 - t0:.2f}s lam {t2 - t1:.2f}s P {t3 - t2:.2f}s gal {t4 - t3:.2f}s]",
                  flush=True)
        A_dev = A_next
    H.Ac = A_dev
    # host-side view of the SpGEMM phases (Galerkin + SA products), then drop the cached
    # scratch blocks (several GB at C4) so the cycle phase does not hold them
    H.spgemm_phases_ms = _setup_phases(reset=True)
    call("mlamg_scratch_trim", None)
    return tm
