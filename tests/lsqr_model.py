"""TEST INFRASTRUCTURE: a host model of the device LSQR (csrc/lsqr.hip) and of the singular
two-level solve built on it, shared by tests/test_lsqr_model_host.py and tests/test_gpu_lsqr.py.

* `sum_512`, `sumsq_512`, `norm_512`: the fixed reduction order of csrc/reduce.hpp on LSQR's grid
  (kSumGrid = 512 workgroups of 256 threads, finished by 256 threads), spelled over the live
  entries only. Steps 2 to 4 are tests/reduce_order.py's own functions.
* `lsqr`: scipy.sparse.linalg.lsqr (scipy 1.15, damp = 0, x0 = 0, calc_var off) restated
  expression for expression, with two things pluggable. `norm` is np.linalg.norm in scipy and
  the fixed-order reduction on the device. `square` is `v**2` in scipy, which CPython and numpy
  both hand to libm's pow, and `v*v` on the device. pow(v, 2) is not always the correctly rounded
  product (it differs from v*v for about 8 doubles in 10,000), and the squares feed only the
  scalars of the stopping tests (anorm, xnorm, rnorm, acond), never x. With scipy's two the model
  is scipy bit for bit; with the device's two it is what mlamg_lsqr must return bit for bit.
* `CASES`: the inputs of both test files, by name, with the stop code each is built to reach.
* `singular_cycle`: oracle.restated.amg_2_v's singular branch with the device's coarse solve,
  mean and error norm substituted.
"""
import functools
from math import sqrt

import numpy as np
import scipy.sparse as sp

from reduce_order import block_totals, partials_total, sumsq_ref

eps = np.finfo(np.float64).eps
SUM_GRID = 512                 # reduce.hpp kSumGrid
SUM_WIDTH = SUM_GRID * 256     # entries one pass of the grid covers


# ---------------------------------------------------------------- the reduction order
def sum_512(vals):
    """Steps 1 to 4 of reduce.hpp for kSumGrid workgroups of 256 threads and a 256-thread
    finish: bitwise reduce_order.sum_ref, without its 131,072-wide arrays for a short vector."""
    vals = np.asarray(vals, dtype=np.float64)
    n = len(vals)
    live = min(n, SUM_WIDTH)
    s = 0.0 + vals[:live]  # step 1: each accumulator starts at +0.0
    for off in range(SUM_WIDTH, n, SUM_WIDTH):
        k = min(SUM_WIDTH, n - off)
        s[:k] = s[:k] + vals[off:off + k]
    nb = max(1, -(-live // 256))  # workgroups with a live thread; the rest hold +0.0 throughout
    threads = np.zeros(nb * 256)
    threads[:live] = s
    partial = np.zeros(SUM_GRID)
    partial[:nb] = block_totals(threads.reshape(nb, 256))
    return partials_total(partial, 256)


def sumsq_512(a):
    a = np.asarray(a, dtype=np.float64)
    return sum_512(a * a)


def norm_512(a):
    """||a|| as k_ls_u / k_ls_v / k_ls_update / k_ls_sq sum it, then one sqrt."""
    return np.sqrt(sumsq_512(a))


def square_mul(v):
    return v * v


def square_pow(v):
    return v**2


# ---------------------------------------------------------------- scipy's LSQR
def _sym_ortho(a, b):
    if b == 0:
        return np.sign(a), 0, abs(a)
    elif a == 0:
        return 0, np.sign(b), abs(b)
    elif abs(b) > abs(a):
        tau = a / b
        s = np.sign(b) / sqrt(1 + tau * tau)
        c = s * tau
        r = b / s
    else:
        tau = b / a
        c = np.sign(a) / sqrt(1 + tau * tau)
        s = c * tau
        r = a / c
    return c, s, r


def lsqr(A, b, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=None, norm=norm_512,
         square=square_mul):
    """scipy.sparse.linalg.lsqr(A, b, atol=, btol=, conlim=, iter_lim=)[:3] -> (x, istop, itn),
    every statement scipy's in scipy's order; matvec is A @ v, rmatvec is A.T.tocsr() @ u (the
    same sums in the same order as scipy's CSC product). Defaults: the device's norm and
    square."""
    A = sp.csr_matrix(A)
    AT = A.T.tocsr()
    b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    if iter_lim is None:
        iter_lim = 2 * n

    itn = 0
    istop = 0
    ctol = 0
    if conlim > 0:
        ctol = 1 / conlim
    anorm = 0
    ddnorm = 0
    res2 = 0
    xnorm = 0
    xxnorm = 0
    z = 0
    cs2 = -1
    sn2 = 0
    dampsq = 0.0

    u = b
    bnorm = norm(b)
    x = np.zeros(n)
    beta = bnorm

    if beta > 0:
        u = (1 / beta) * u
        v = AT @ u
        alfa = norm(v)
    else:
        v = x.copy()
        alfa = 0

    if alfa > 0:
        v = (1 / alfa) * v
    w = v.copy()

    rhobar = alfa
    phibar = beta

    arnorm = alfa * beta
    if arnorm == 0:
        return x, istop, itn

    while itn < iter_lim:
        itn = itn + 1
        u = A @ v - alfa * u
        beta = norm(u)

        if beta > 0:
            u = (1 / beta) * u
            anorm = sqrt(square(anorm) + square(alfa) + square(beta) + dampsq)
            v = AT @ u - beta * v
            alfa = norm(v)
            if alfa > 0:
                v = (1 / alfa) * v

        rhobar1 = rhobar
        psi = 0.

        cs, sn, rho = _sym_ortho(rhobar1, beta)

        theta = sn * alfa
        rhobar = -cs * alfa
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi

        t1 = phi / rho
        t2 = -theta / rho
        dk = (1 / rho) * w

        x = x + t1 * w
        w = v + t2 * w
        ddnorm = ddnorm + square(norm(dk))

        delta = sn2 * rho
        gambar = -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = sqrt(xxnorm + square(zbar))
        gamma = sqrt(square(gambar) + square(theta))
        cs2 = gambar / gamma
        sn2 = theta / gamma
        z = rhs / gamma
        xxnorm = xxnorm + square(z)

        acond = anorm * sqrt(ddnorm)
        res1 = square(phibar)
        res2 = res2 + square(psi)
        rnorm = sqrt(res1 + res2)
        arnorm = alfa * abs(tau)

        test1 = rnorm / bnorm
        test2 = arnorm / (anorm * rnorm + eps)
        test3 = 1 / (acond + eps)
        t1 = test1 / (1 + anorm * xnorm / bnorm)
        rtol = btol + atol * anorm * xnorm / bnorm

        if itn >= iter_lim:
            istop = 7
        if 1 + test3 <= 1:
            istop = 6
        if 1 + test2 <= 1:
            istop = 5
        if 1 + t1 <= 1:
            istop = 4

        if test3 <= ctol:
            istop = 3
        if test2 <= atol:
            istop = 2
        if test1 <= rtol:
            istop = 1

        if istop != 0:
            break

    return x, istop, itn


# ---------------------------------------------------------------- the cases
def neumann_1d(n):
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    return sp.diags([-np.ones(n - 1), d, -np.ones(n - 1)], [-1, 0, 1], format="csr")


def neumann_2d(ny, nx):
    """The five-point Neumann Laplacian on an ny x nx grid: singular, constant nullspace."""
    A = (sp.kron(sp.eye(ny), neumann_1d(nx)) + sp.kron(neumann_1d(ny), sp.eye(nx))).tocsr()
    A.sort_indices()
    return A


def _canonical(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def _tall():
    rs = np.random.RandomState(3)
    A = _canonical(sp.random(300, 120, density=0.05, random_state=rs, format="csr")
                   + sp.eye(300, 120, format="csr"))
    return A, A @ rs.randn(120), rs.randn(300)


def _mean_free(rs, n):
    b = rs.randn(n)
    return b - b.mean()


def _case_tall(consistent, **kw):
    A, bc, bi = _tall()
    return A, (bc if consistent else bi), kw


def _case_wide():
    rs = np.random.RandomState(4)
    A = _canonical(sp.random(90, 260, density=0.06, random_state=rs, format="csr")
                   + sp.eye(90, 260, format="csr"))
    return A, rs.randn(90), {}


def _case_neumann(shift):
    A = neumann_2d(17, 13)
    return A, _mean_free(np.random.RandomState(5), A.shape[0]) + shift, {}


def _case_conlim():
    A = sp.diags(np.logspace(0, -10, 200), format="csr")
    return A, A @ np.ones(200), dict(atol=1e-14, btol=1e-14, conlim=1e4)


def _case_three_values():
    A = sp.diags(np.repeat([1.0, 2.0, 4.0], 50), format="csr")
    return A, np.random.RandomState(6).randn(150), dict(atol=0, btol=0, conlim=0)


def _case_tiny_rhs():
    """One singular value and ||b|| about 1e-39: after the one step that solves it, test 5 holds
    (arnorm is far under the absolute eps of test2's denominator) and so does test 4 (t1 is
    2.5e-17, under eps / 2), so the code is 4 only because test 4 is applied after test 5."""
    A = sp.diags(np.full(50, 2.5), format="csr")
    return A, 1e-40 * np.random.RandomState(8).randn(50), dict(atol=0, btol=0, conlim=0)


def _case_tiny_rhs_atol():
    """The same system with conlim = 0.5 (test 3 holds: acond is 1), atol = 1e-30 (test 2 holds:
    test2 is 4e-40) and btol = 0 (test 1 does not: test1 is 5e-17, rtol 1e-30): the code is 2
    only because test 2 is applied after tests 5, 4 and 3."""
    A, b, _ = _case_tiny_rhs()
    return A, b, dict(atol=1e-30, btol=0, conlim=0.5)


def _case_one_by_one():
    return sp.csr_matrix(np.array([[2.5]])), np.array([1.0]), {}


def _case_zero_matrix():
    return sp.csr_matrix((5, 4), dtype=np.float64), np.ones(5), {}


def _case_emptied_row():
    A = _tall()[0].tolil()
    A[7, :] = 0
    A = _canonical(A.tocsr())
    A.eliminate_zeros()
    b = np.zeros(300)
    b[7] = 1.0
    return A, b, {}


def _case_long():
    A = neumann_2d(400, 350)
    return A, _mean_free(np.random.RandomState(7), A.shape[0]), dict(iter_lim=20)


MACHINE = dict(atol=0, btol=0, conlim=0)
# name -> (constructor of (A, b, kwargs), the stop code it is built to reach, itn or None)
CASES = {
    "tall_consistent": (functools.partial(_case_tall, True), 1, None),
    "tall_inconsistent": (functools.partial(_case_tall, False), 2, None),
    "wide": (_case_wide, 1, None),
    "neumann_consistent": (functools.partial(_case_neumann, 0.0), 1, None),
    "neumann_inconsistent": (functools.partial(_case_neumann, 0.3), 2, None),
    "machine_consistent": (functools.partial(_case_tall, True, **MACHINE), 4, None),
    "machine_inconsistent": (functools.partial(_case_tall, False, **MACHINE), 5, None),
    "condition_limit": (_case_conlim, 3, None),
    "three_singular_values": (_case_three_values, 4, 4),
    "tiny_rhs": (_case_tiny_rhs, 4, 1),
    "tiny_rhs_atol": (_case_tiny_rhs_atol, 2, 1),
    # test 1 holds on the very iteration that reaches iter_lim: 1 is applied after 7
    "limit_and_converged": (functools.partial(_case_tall, True, iter_lim=28), 1, 28),
    "one_by_one": (_case_one_by_one, 1, 1),
    "zero_matrix": (_case_zero_matrix, 0, 0),
    "b_on_emptied_row": (_case_emptied_row, 0, 0),
    "long_vectors": (_case_long, 7, 20),
}
for _k in (1, 7, 8, 9, 17):  # either side of the host's poll of the flag every 8 iterations
    CASES[f"iteration_limit_{_k}"] = (
        functools.partial(_case_tall, False, iter_lim=_k, atol=1e-12, btol=1e-12), 7, _k)


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, b, kwargs) of the case, built once. Treat as read-only."""
    A, b, kw = CASES[name][0]()
    b.setflags(write=False)
    return A, b, kw


@functools.lru_cache(maxsize=None)
def model(name):
    """The device-order model's (x, istop, itn) on the case, computed once."""
    A, b, kw = case(name)
    x, istop, itn = lsqr(A, b, **kw)
    x.setflags(write=False)
    return x, istop, itn


# ---------------------------------------------------------------- the singular cycle
def singular_cycle(A, P, b, x0, nu_pre=1, nu_post=1, smoother="gauss_seidel", jacobi_weight=0.666,
                   tol=0.0, res_tol_mode=False, max_iter=500):
    """oracle.restated.amg_2_v(..., singular=True) with the device's three reductions:
      * the coarse solve is `lsqr` above (device norm and square, scipy's defaults otherwise) on
        the canonical P.T @ A @ P;
      * x -= mean(x) is x - sum_512(x) / n (mlamg_remove_mean);
      * the error norm is sqrt(sumsq_ref(x)) (mlamg_norm2's grid, capped at 1024).
    The residual norm of res_tol_mode stays np.linalg.norm(b - A @ x): the device's fused
    residual norm has a format-dependent order and is held to a bound, not to bits.
    Returns (x, err history, [(istop, itn) of each cycle's coarse solve])."""
    from oracle import restated
    A = sp.csr_matrix(A)
    P = sp.csr_matrix(P)
    A_H = restated.galerkin(A, P)
    n = A.shape[0]
    x = np.array(x0, dtype=np.float64)
    if smoother == "jacobi":
        Dw = restated.mlamg_dinv(A, jacobi_weight)

        def smooth(nu):
            restated.jacobi_mlamg(A, Dw, b, x, nu)
    else:
        def smooth(nu):
            restated.gauss_seidel(A, x, b, iterations=nu)
    err = np.zeros(max_iter)
    stops = []
    for i in range(max_iter):
        smooth(nu_pre)
        e_H, istop, itn = lsqr(A_H, P.T @ (b - A @ x))
        stops.append((istop, itn))
        x += P @ e_H
        smooth(nu_post)
        x[...] = x - sum_512(x) / float(n)
        if res_tol_mode:
            e = np.linalg.norm(b - A @ x, 2)
        else:
            e = np.sqrt(sumsq_ref(x))
        err[i] = e
        if e <= tol:
            err = err[:i + 1]
            break
    return x, err, stops
