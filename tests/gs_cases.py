"""The Gauss-Seidel test matrices and the path each takes (mlamg_gs_path), shared
by the host planner's test (test_gs_plan_host.py, CPU) and the sweeps' tests (test_gpu_kernels.py).
The table is the issue's; the planner run on the CPU is what the GPU tests then assert."""
import functools

import numpy as np
import scipy.sparse as sp

# mlamg_gs_path values (include/mlamg.h)
LEVELS, WORKGROUP, WAVE, WRING, PIPE, PIPE_LDS, RING, WINDOW = range(8)
PATH_NAMES = ("LEVELS", "WORKGROUP", "WAVE", "WRING", "PIPE", "PIPE_LDS", "RING", "WINDOW")


def poisson_2d(m):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    return (sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m))).tocsr()


def poisson_3d(m):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    return (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()


def nine_point(m):
    T = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(m, m))
    return (sp.kron(T, T) * -1.0 + sp.eye(m * m) * 9.0).tocsr()


def long_rows(m):
    """25-point stencil: 24 off-diagonals in the interior."""
    T = sp.diags([1.0, 1.0, 1.0, 1.0, 1.0], [-2, -1, 0, 1, 2], shape=(m, m))
    return (sp.kron(T, T) * -0.1 + sp.eye(m * m) * 4.0).tocsr()


def unsorted_zero_diag(m):
    """5-point grid with a zero diagonal (row 100: left alone by gauss_seidel), every third row
    stored in descending column order and row 7's diagonal stored twice (the last one counts)."""
    A = poisson_2d(m).tolil()
    A[100, 100] = 0.0
    A = A.tocsr()
    A.sort_indices()
    ip, ij, ax = A.indptr.copy(), A.indices.copy(), A.data.copy()
    for r in range(0, A.shape[0], 3):
        ij[ip[r]:ip[r + 1]] = ij[ip[r]:ip[r + 1]][::-1].copy()
        ax[ip[r]:ip[r + 1]] = ax[ip[r]:ip[r + 1]][::-1].copy()
    ij = np.concatenate([ij[:ip[8]], [7], ij[ip[8]:]]).astype(np.int32)
    ax = np.concatenate([ax[:ip[8]], [5.0], ax[ip[8]:]])
    ip[8:] += 1
    return sp.csr_matrix((ax, ij, ip), shape=A.shape)


@functools.lru_cache(maxsize=None)
def wide_levels(seed=11):
    """Diagonal + a sparse upper band: a few levels of ~10^4 independent rows. Drawing the
    pattern takes half a minute, so the matrix is built once per process: callers copy it."""
    n = 30000
    U = sp.random(n, n, density=2e-5, random_state=np.random.RandomState(seed), format="csr")
    return (sp.eye(n) * 4.0 + sp.triu(U, k=1) - sp.triu(U, k=1).T).tocsr()


def slab(levels, width):
    """kron(tridiag(levels), I_width): `levels` levels of `width` rows, 2 off-diagonals a row."""
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(levels, levels))
    return sp.kron(T, sp.identity(width)).tocsr()


def band(n, half):
    """Dense band: up to 2 * half + 1 entries a row, n levels of one row."""
    offs = list(range(-half, half + 1))
    return sp.diags([np.full(n - abs(o), 10.0 * half if o == 0 else -1.0 / (1 + abs(o)))
                     for o in offs], offs, shape=(n, n)).tocsr()


def sorted_csr(A):
    A = sp.csr_matrix(A, copy=True)
    A.sort_indices()
    return A


# test_gauss_seidel_both_schedules' cases: name -> (matrix builder, path)
BOTH_SCHEDULES = {
    "wide_levels": (lambda: sorted_csr(wide_levels()), LEVELS),
    "grid_200": (lambda: sorted_csr(poisson_2d(200)), WINDOW),
    "grid_1100": (lambda: sorted_csr(poisson_2d(1100)), PIPE),  # R = 2, K = 4
    "cube_24": (lambda: sorted_csr(poisson_3d(24)), WINDOW),
    "long_rows": (lambda: sorted_csr(long_rows(60)), WRING),  # lpr 16, epl 2
    "unsorted_zero_diag": (lambda: unsorted_zero_diag(64), WINDOW),
    "grid_60_lds": (lambda: sorted_csr(poisson_2d(60)), WINDOW),
    "cube_12_lds": (lambda: sorted_csr(poisson_3d(12)), WINDOW),
    "grid_256": (lambda: sorted_csr(poisson_2d(256)), WINDOW),
    "nine_point_48": (lambda: sorted_csr(nine_point(48)), WINDOW),
    "grid_160": (lambda: sorted_csr(poisson_2d(160)), WINDOW),
    "grid_400": (lambda: sorted_csr(poisson_2d(400)), WINDOW),
    "nine_point_300": (lambda: sorted_csr(nine_point(300)), WINDOW),
}

# test_gauss_seidel_every_path's cases: name -> (matrix builder, knobs set to 1, path); the paths
# the cases above do not reach, each at most 9,000 rows
EVERY_PATH = {
    "ring_slab_600": (lambda: slab(6, 600), (), RING),
    "ring_grid_60": (lambda: sorted_csr(poisson_2d(60)), ("NO_WIN",), RING),
    "ring_unsorted_64": (lambda: unsorted_zero_diag(64), ("NO_WIN",), RING),
    "lds_k4_grid_60": (lambda: sorted_csr(poisson_2d(60)), ("NO_WIN", "NO_RING"), PIPE_LDS),
    "lds_k8_cube_12": (lambda: sorted_csr(poisson_3d(12)), ("NO_WIN",), PIPE_LDS),
    "lds_unsorted_64": (lambda: unsorted_zero_diag(64), ("NO_WIN", "NO_RING"), PIPE_LDS),
    "pipe_r1_k4_grid_60": (lambda: sorted_csr(poisson_2d(60)), ("NO_WIN", "NO_RING", "NO_LDS"),
                           PIPE),
    "pipe_r1_k8_cube_12": (lambda: sorted_csr(poisson_3d(12)), ("NO_WIN", "NO_LDS"), PIPE),
    "pipe_r1_unsorted_64": (lambda: unsorted_zero_diag(64), ("NO_WIN", "NO_RING", "NO_LDS"), PIPE),
    "pipe_r2_slab_1500": (lambda: slab(6, 1500), (), PIPE),
    "wave_band_40": (lambda: band(600, 40), (), WAVE),  # 81 entries a row
    "wave_long_rows_24": (lambda: sorted_csr(long_rows(24)), ("NO_WRING",), WAVE),
    "workgroup_band_70": (lambda: band(400, 70), (), WORKGROUP),  # 141 entries a row
    "workgroup_long_rows_24": (lambda: sorted_csr(long_rows(24)), ("NO_WRING", "NO_WAVE"),
                               WORKGROUP),
}
