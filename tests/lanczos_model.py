"""TEST INFRASTRUCTURE: lambda_max(D^-1 A) three ways, shared by tests/test_lambda_max_host.py,
tests/test_tridiag_host.py and tests/test_gpu_lambda_max.py.

* `lanczos`: a plain numpy restatement of mlamg_lambda_max_dinvA (csrc/eig.hip with
  csrc/tridiag.hpp): the splitmix start vector, the recurrence in the D inner product, the read
  of T every 32 steps, the breakdown rule, the stagnation test and the bad-diagonal guard. Only
  the order of the sums differs from the device (numpy's instead of the fixed block order).
* `CASES`: the matrices whose lambda_max is held to BOUND, by name.
* `reference`: the largest eigenvalue of S = D^-1/2 A D^-1/2 by LAPACK on the dense (or
  tridiagonal) S; `poisson_closed_form` and `reference_mp` are the checks of that reference.
"""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp

BOUND = 1e-12  # relative, on lambda_max and so on omega = (4/3)/lambda_max
CHECK = 32     # eig.hip kCheck


class BadDiagonal(ValueError):
    """The device's MLAMG_EINVAL for a diagonal the D inner product cannot take."""


# ---------------------------------------------------------------- the restatement
def splitmix_start(n, seed):
    """k_lz_init's start vector: splitmix64 of seed * 0x100000001B3 + i, mapped to [-1, 1)."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) * np.uint64(0x100000001B3) + np.arange(n, dtype=np.uint64)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) * 2.0 - 1.0


def sturm_count(a, b, m, x):
    """csrc/tridiag.hpp sturm_count: eigenvalues of (a[0..m), b[1..m)) smaller than x."""
    cnt = 0
    q = 1.0
    for i in range(m):
        q = (a[i] - x) - (b[i] * b[i] / q if i > 0 else 0.0)
        if q == 0.0:
            q = -1e-300
        if q < 0.0:
            cnt += 1
    return cnt


def tridiag_max_eig(a, b, m):
    """csrc/tridiag.hpp tridiag_max_eig: Gershgorin bracket, then bisection."""
    lo = hi = a[0]
    for i in range(m):
        r = (abs(b[i]) if i > 0 else 0.0) + (abs(b[i + 1]) if i + 1 < m else 0.0)
        lo = min(lo, a[i] - r)
        hi = max(hi, a[i] + r)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if sturm_count(a, b, m, mid) == m:
            hi = mid
        else:
            lo = mid
    return hi


def stored_diagonal(A):
    """(d, stored): the sum of each row's stored diagonal entries, and whether it has any."""
    A = A.tocsr()
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    on = A.indices == rows
    d = np.bincount(rows[on], weights=A.data[on], minlength=n).astype(np.float64)
    return d, np.bincount(rows[on], minlength=n) > 0


def lanczos(A, max_iter=20000, tol=1e-15, seed=0):
    """mlamg_lambda_max_dinvA restated -> (lambda, iters, alpha, beta, m): alpha[0..iters) and
    beta[0..iters] as the host read them last, m the rows of T that gave lambda."""
    A = A.tocsr()
    n = A.shape[0]
    if n == 0:
        return 0.0, 0, [], [0.0], 0
    d, stored = stored_diagonal(A)
    with np.errstate(divide="ignore", invalid="ignore"):
        dinv = 1.0 / d
    for bad, what in ((~stored, "a row has no stored diagonal entry"),
                      (stored & (d == 0.0), "a row has a zero diagonal entry"),
                      (d < 0.0, "a row has a negative diagonal entry"),
                      (~np.isfinite(d), "a row has a non-finite diagonal entry")):
        if bad.any():
            raise BadDiagonal(what)
    q = splitmix_start(n, seed)
    nrm0 = np.sqrt(np.sum(d * (q * q)))
    q = q * (1.0 / nrm0 if nrm0 > 0.0 else 0.0)
    qprev = np.zeros(n)
    ha, hb = [], [0.0]
    theta_prev, theta = -1.0, 0.0
    j = 0
    while True:
        jend = min(max_iter, j + CHECK)  # no cap at n
        while j < jend:
            z = A @ q
            a = float(np.sum(z * q))
            w = (dinv * z - a * q) - hb[j] * qprev
            b = float(np.sqrt(np.sum(d * (w * w))))
            ha.append(a)
            hb.append(b)
            qprev, q = q, w * (1.0 / b if b > 0.0 else 0.0)
            j += 1
        m, breakdown = j, False
        for i in range(1, j + 1):
            if not (hb[i] > 1e-14 * abs(ha[i - 1]) + 1e-300):
                m, breakdown = i, True
                break
        theta = tridiag_max_eig(ha, hb, m)
        done = breakdown or j >= max_iter
        if theta_prev > 0.0 and abs(theta - theta_prev) <= tol * abs(theta):
            done = True
        theta_prev = theta
        if done:
            if not np.isfinite(theta):
                raise BadDiagonal("non-finite result")
            return theta, j, ha, hb, m


# ---------------------------------------------------------------- the matrices
def tridiag_from_faces(c):
    """1D diffusion with face coefficients c[0..n]: tridiag(-c[1:-1], c[:-1] + c[1:], -c[1:-1])."""
    return sp.diags([-c[1:-1], c[:-1] + c[1:], -c[1:-1]], [-1, 0, 1], format="csr")


@functools.lru_cache(maxsize=None)
def _jump_faces():
    rs = np.random.RandomState(0)  # n = 64 first, n = 150 from the next draw
    return {n: 10.0 ** rs.uniform(-2, 2, n + 1) for n in (64, 150)}


def jump_1d(n):
    """1D diffusion, face coefficients 10^U(-2, 2): loses orthogonality well before n steps."""
    return tridiag_from_faces(_jump_faces()[n])


def poisson_1d(n):
    return tridiag_from_faces(np.ones(n + 1))


def diagonal(n=40):
    return sp.diags([np.linspace(0.5, 7.0, n)], [0], format="csr")


def four_blocks():
    """Four identical 50-row blocks (a 5 x 10 five-point grid each): multiplicity 4."""
    from mlamg import problems
    return sp.block_diag([problems.poisson_2d_5pt(5, 10)] * 4, format="csr")


def top_cluster(n=200):
    """S with unit diagonal and eigenvalues 2, 2 - 5e-7, 2 - 1e-6 above a spread of 197 (a dense
    orthogonal similarity of the diagonal matrix: scipy's random correlation matrix), then
    A = D^1/2 S D^1/2 with a diagonal over two decades. Dense, stored as CSR."""
    import scipy.stats
    low = np.linspace(0.1, 1.0, n - 3)
    top = np.array([2.0 - 1e-6, 2.0 - 5e-7, 2.0])
    low *= (n - top.sum()) / low.sum()
    S = scipy.stats.random_correlation.rvs(np.concatenate([low, top]), random_state=7)
    r = np.sqrt(10.0 ** np.random.RandomState(7).uniform(-1, 1, n))
    A = S * r[:, None] * r[None, :]
    return sp.csr_matrix(0.5 * (A + A.T))


def _level0(name):
    from mlamg import problems
    if name == "p2d48":
        return problems.poisson_2d_5pt(48), 48
    if name == "jump2d48":
        jumps = problems.voronoi_jumps(np.random.RandomState(0))
        return problems.jump_2d(48, jumps), 48
    return jump_1d(150), None


@functools.lru_cache(maxsize=None)
def galerkin_levels(name):
    """Three levels under box aggregates of size 3, every step the oracle's own
    (smoothed_aggregation_jacobi, galerkin), omega from `reference` so that nothing here depends
    on ARPACK's start vector. In 2D the coarse rows are wider than any level-0 row."""
    from mlamg import problems
    from oracle import restated
    A, nx = _level0(name)
    A = restated.canonical(A)
    out = [A]
    for _ in range(2):
        n = A.shape[0]
        Agg = (problems.box_aggregates_1d(n, 3) if nx is None
               else problems.box_aggregates_2d(nx, size=3))
        P, _ = restated.smoothed_aggregation_jacobi(A, Agg, omega=(4.0 / 3.0) / _lambda_ref(A))
        A = restated.galerkin(A, sp.csr_matrix(P))
        nx = None if nx is None else (nx + 2) // 3
        out.append(A)
    return out


def reversed_columns():
    """The n = 64 jump matrix with every row's entries stored in descending column order."""
    A = jump_1d(64)
    ip = A.indptr
    idx = np.concatenate([np.arange(ip[i + 1] - 1, ip[i] - 1, -1) for i in range(A.shape[0])])
    B = sp.csr_matrix((A.data[idx], A.indices[idx], ip.copy()), shape=A.shape)
    return B


def split_diagonal():
    """The 12 x 12 five-point grid with every diagonal entry stored twice (1/4 and 3/4 of it,
    exact in binary) at the two ends of its row: k_lz_init has to sum the stored entries."""
    from mlamg import problems
    A = problems.poisson_2d_5pt(12).tocsr()
    A.sort_indices()
    n = A.shape[0]
    ip, ij, ax = [0], [], []
    for i in range(n):
        c, v = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
        off = c != i
        dii = v[~off].sum()
        ij += [i] + list(c[off]) + [i]
        ax += [0.25 * dii] + list(v[off]) + [0.75 * dii]
        ip.append(len(ij))
    return sp.csr_matrix((np.array(ax), np.array(ij, dtype=np.int32), np.array(ip, dtype=np.int32)),
                         shape=A.shape)


def with_diagonal(A, rows, value):
    """A with the stored diagonal entries of `rows` set to value (None: not stored at all)."""
    A = A.tocoo()
    on = (A.row == A.col) & np.isin(A.row, rows)
    data = A.data.copy()
    keep = ~on if value is None else np.ones(len(data), dtype=bool)
    if value is not None:
        data[on] = value
    return sp.csr_matrix((data[keep], (A.row[keep], A.col[keep])), shape=A.shape)


# diagonals that the D inner product cannot take, in the last rows (the last block of k_lz_init)
BAD_DIAGONALS = {
    "zero": lambda A: with_diagonal(A, [A.shape[0] - 3], 0.0),
    "missing": lambda A: with_diagonal(A, [A.shape[0] - 3], None),
    "mixed_sign": lambda A: with_diagonal(A, [A.shape[0] - 3, A.shape[0] - 2], -2.0),
    "all_negative": lambda A: sp.csr_matrix(-A),
    "nan": lambda A: with_diagonal(A, [A.shape[0] - 3], np.nan),
}


CASES = {
    "jump1d_64": lambda: jump_1d(64),
    "jump1d_150": lambda: jump_1d(150),
    "poisson1d_2000": lambda: poisson_1d(2000),
    "poisson1d_33": lambda: poisson_1d(33),
    "poisson1d_65": lambda: poisson_1d(65),
    "poisson1d_1": lambda: poisson_1d(1),
    "poisson1d_2": lambda: poisson_1d(2),
    "poisson1d_3": lambda: poisson_1d(3),
    "poisson1d_5": lambda: poisson_1d(5),
    "diagonal_40": diagonal,
    "four_blocks_50": four_blocks,
    "top_cluster_200": top_cluster,
    "reversed_columns_64": reversed_columns,
    "split_diagonal_144": split_diagonal,
}
def _level(h, l):
    return galerkin_levels(h)[l]


for _h in ("p2d48", "jump2d48", "jump1d150"):
    for _l in range(3):
        CASES[f"galerkin_{_h}_L{_l}"] = functools.partial(_level, _h, _l)
POISSON_1D = {name: int(name.split("_")[1]) for name in CASES if name.startswith("poisson1d_")}
TINY = ("poisson1d_1", "poisson1d_2", "poisson1d_3", "poisson1d_5")


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The case's matrix, built once. Treat as read-only."""
    return CASES[name]()


# ---------------------------------------------------------------- the references
def scaled_dense(A):
    """S = D^-1/2 A D^-1/2 as a dense array (duplicate entries summed, as scipy does)."""
    M = A.toarray()
    r = 1.0 / np.sqrt(np.diag(M))
    return M * r[:, None] * r[None, :]


def _lambda_ref(A):
    S = scaled_dense(A)
    n = S.shape[0]
    if n == 1:
        return float(S[0, 0])
    if not np.any(np.triu(S, 2)) and not np.any(np.tril(S, -2)):
        return float(scipy.linalg.eigvalsh_tridiagonal(
            np.diag(S).copy(), np.diag(S, -1).copy(), select="i", select_range=(n - 1, n - 1))[0])
    return float(scipy.linalg.eigvalsh(S, subset_by_index=(n - 1, n - 1))[0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """lambda_max(D^-1 A) of the case: the largest eigenvalue of S by LAPACK, in fp64."""
    return _lambda_ref(matrix(name))


def poisson_closed_form(n):
    """1 + cos(pi / (n + 1)), evaluated at 50 digits and rounded once."""
    import mpmath
    with mpmath.workdps(50):
        return float(1 + mpmath.cos(mpmath.pi / (n + 1)))


def reference_mp(A, digits=50):
    """The largest eigenvalue of S at `digits` digits (mpmath.eigsy; small matrices only): S is
    formed from the fp64 entries of A exactly, so this referees `reference`'s rounding."""
    import mpmath
    M = A.toarray()
    with mpmath.workdps(digits):
        n = M.shape[0]
        r = [1 / mpmath.sqrt(mpmath.mpf(float(M[i, i]))) for i in range(n)]
        S = mpmath.matrix(n, n)
        for i, j in zip(*np.nonzero(M)):
            S[int(i), int(j)] = mpmath.mpf(float(M[i, j])) * r[i] * r[j]
        ev = mpmath.eigsy(S, eigvals_only=True)
        return float(max(ev))
