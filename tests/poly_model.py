"""Host model of the polynomial (Chebyshev) smoother and of the V-cycles built on it: numpy, with
scipy's csr_matvec for every A @ v, so that each operation rounds exactly as pyamg's
relaxation.polynomial does (restated from pyamg 4.x):

    repeat `iterations` times:
        r = b - A @ x
        h = c[0] * r
        for c_i in c[1:]:  h = c_i * r + A @ h
        x += h
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse import _sparsetools


def matvec(A, x):
    """A @ x by scipy's csr_matvec: each row summed left to right in stored order from +0.0."""
    y = np.zeros(A.shape[0], dtype=np.float64)
    _sparsetools.csr_matvec(A.shape[0], A.shape[1], A.indptr, A.indices, A.data,
                            np.ascontiguousarray(x, dtype=np.float64), y)
    return y


def sweep(A, x, b, coefficients, iterations=1, x_is_zero=False):
    """The sweep above on a copy of x (b None: a zero right-hand side). x_is_zero: x is not
    read; the first residual is b itself and the first update adds to +0.0."""
    c = np.asarray(coefficients, dtype=np.float64)
    assert c.ndim == 1 and c.size >= 1
    n = A.shape[0]
    b = np.zeros(n) if b is None else np.asarray(b, dtype=np.float64)
    x = np.zeros(n) if x_is_zero else np.array(x, dtype=np.float64, copy=True)
    for it in range(iterations):
        if x_is_zero and it == 0:
            r = b.copy()
        else:
            r = b - matvec(A, x)
        h = c[0] * r
        for ci in c[1:]:
            t = ci * r
            h = t + matvec(A, h)
        x = x + h
    return x


def vcycle(levels, coarse, b, x, nu_pre=1, nu_post=1, lvl=0):
    """One V(nu_pre, nu_post) cycle. levels: dicts with A, P, R (scipy CSR), c (coefficients) and
    iters (iterations per sweep); coarse: the dense matrix applied on the coarsest level (a
    pseudo-inverse). Levels below the first start from a zero guess, as the executors do."""
    if lvl == len(levels):
        return coarse @ b
    L = levels[lvl]
    if nu_pre > 0:
        x = sweep(L["A"], x, b, L["c"], nu_pre * L["iters"])
    r = b - matvec(L["A"], x)
    bc = matvec(L["R"], r)
    ec = vcycle(levels, coarse, bc, np.zeros(bc.size), nu_pre, nu_post, lvl + 1)
    x = x + matvec(L["P"], ec)
    if nu_post > 0:
        x = sweep(L["A"], x, b, L["c"], nu_post * L["iters"])
    return x


def cycles(levels, coarse, b, x, n_cycles, nu_pre=1, nu_post=1):
    for _ in range(n_cycles):
        x = vcycle(levels, coarse, b, x, nu_pre, nu_post)
    return x


def model_levels(H, iterations=1):
    """The model's levels from a device hierarchy whose levels carry polynomial smoothers."""
    out = []
    for L in H.levels:
        out.append({"A": sp.csr_matrix(L.A.to_scipy()), "P": sp.csr_matrix(L.P.to_scipy()),
                    "R": sp.csr_matrix(L.R.to_scipy()),
                    "c": np.array(L.poly.coefficients, copy=True), "iters": iterations})
    return out
