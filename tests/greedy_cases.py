"""The matrices of the greedy C/F splitting tests, rebuilt from seeds: shared by
tests/test_greedy_host.py, the GPU tests of the learned-P setup and tools/make_greedy_golden.py
(which records the reference's F and C for them into tests/golden/greedy_cf.npz)."""
import numpy as np
import scipy.sparse as sp


def poisson_1d(n):
    A = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def poisson_2d(m):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    A = (sp.kron(I, T) + sp.kron(T, I)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def random_m_matrix(m, seed):
    """Symmetric M-matrix on the 5-point pattern of the m x m grid: off-diagonals -w_ij with
    w uniform in [0.1, 1), diagonal (1 + u_i) times the row's off-diagonal sum, u uniform in
    [0, 0.5): initial dominances spread over [0.5, 0.6]."""
    rs = np.random.RandomState(seed)
    P = sp.triu(poisson_2d(m), k=1).tocoo()
    w = rs.uniform(0.1, 1.0, P.nnz)
    O = sp.coo_matrix((-w, (P.row, P.col)), shape=P.shape)
    O = (O + O.T).tocsr()
    s = np.asarray(abs(O).sum(axis=1)).ravel()
    A = (O + sp.diags(s * (1.0 + rs.uniform(0.0, 0.5, m * m)))).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def all_fine(n):
    A = sp.diags([-0.1, 4.0, -0.1], [-1, 0, 1], shape=(n, n)).tocsr()
    A.sort_indices()
    return A


# name -> (builder, theta, exact sums: the integer stencils need no gap check)
CASES = {
    "poisson1d_9": (lambda: poisson_1d(9), 0.56, True),
    "grid_6": (lambda: poisson_2d(6), 0.56, True),
    "grid_12": (lambda: poisson_2d(12), 0.56, True),
    "grid_12_theta07": (lambda: poisson_2d(12), 0.7, True),
    "random_8": (lambda: random_m_matrix(8, 8001), 0.56, False),
    "random_16": (lambda: random_m_matrix(16, 16001), 0.56, False),
    "all_fine_7": (lambda: all_fine(7), 0.56, True),
}
