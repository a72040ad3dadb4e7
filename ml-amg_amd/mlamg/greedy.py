"""Greedy C/F splitting by diagonal dominance: ns/lib/greedy.py greedy_coarsening, step 1 of the
reference preconditioner's setup (ns/preconditioner/MLAMG.py:116). Runs on the host
(csrc/greedy.cpp, no device call) with an ordered set in place of the reference's O(n^2)
setdiff1d loop; F and C come back in the reference's append order (tests/test_greedy_host.py
holds them to the reference's own results)."""
from __future__ import annotations

import ctypes

import numpy as np
import scipy.sparse as sp

from ._lib import call


def greedy_coarsening(A, theta):
    """-> (len(F), F, C) like the reference: F the fine rows, C the coarse rows (int64 arrays,
    append order; the order of C is the column order of the learned P). A: square scipy matrix
    with a nonzero diagonal; it is brought to canonical CSR (sorted, duplicates summed)."""
    A = sp.csr_matrix(A)
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"greedy_coarsening needs a square matrix, got {A.shape}")
    if not A.has_canonical_format:
        A = A.copy()
        A.sum_duplicates()
    n = A.shape[0]
    indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    F = np.empty(max(n, 1), dtype=np.int32)
    C = np.empty(max(n, 1), dtype=np.int32)
    nF, nC = ctypes.c_int64(0), ctypes.c_int64(0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    call("mlamg_greedy_coarsening", n, vp(indptr), vp(indices), vp(data), float(theta), vp(F),
         vp(C), ctypes.cast(ctypes.byref(nF), ctypes.c_void_p),
         ctypes.cast(ctypes.byref(nC), ctypes.c_void_p))
    F, C = F[:nF.value].astype(np.int64), C[:nC.value].astype(np.int64)
    return len(F), F, C
