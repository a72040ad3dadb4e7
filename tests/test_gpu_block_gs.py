"""GPU: Gauss-Seidel on a block of k vectors (mlamg_gs_sweep_mv) and the block
V-cycle with Gauss-Seidel levels (Hierarchy.enable_block_gauss_seidel).

The acceptance criterion is §17's: column j of every block result is bitwise the single-vector
result on column j (mlamg_gs_sweep is itself pinned to the sequential pyamg sweep of
oracle/oracle.c). Every comparison is np.array_equal."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 9, 64)
# mlamg_gs_mv_path: the selection rule walks a schedule in one workgroup when it has more than 4
# levels and max_level_rows * ceil(k / 2) <= WALK_ITEMS on the packed copy, WALK_ITEMS_CSR on the
# CSR arrays (csrc/gs_mv.hip kGsMvWalkItems, kGsMvWalkItemsCsr)
PER_LEVEL, WALK_CSR, WALK_PACKED = 0, 1, 2
WALK_ITEMS = 4 * 1024
WALK_ITEMS_CSR = 2 * 1024


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.hierarchy
    import mlamg.multigrid
    import mlamg.preconditioner
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


def _call(name, *args):
    from mlamg._lib import call
    return call(name, *args)


@functools.lru_cache(maxsize=None)
def _matrix(ml, name):
    """The schedules of tests/test_gpu_kernels.py::test_gauss_seidel_both_schedules that reach
    the three block paths."""
    if name == "grid_60":
        return ml.problems.poisson_2d_5pt(60).tocsr()
    if name == "cube_12":  # 6 off-diagonals: 8 packed slots per row
        return ml.problems.poisson_3d_7pt(12).tocsr()
    if name in ("long_rows_24", "long_rows_240"):  # more than 8 off-diagonals: no packed copy
        m = int(name[10:])
        T = sp.diags([1.0, 1.0, 1.0, 1.0, 1.0], [-2, -1, 0, 1, 2], shape=(m, m))
        return (sp.kron(T, T) * -0.1 + sp.eye(m * m) * 4.0).tocsr()
    if name == "wide_levels":  # diagonal + a sparse upper band: a few levels of ~10^4 rows
        # (that test's construction with the 18,000 entries of U drawn directly: sp.random
        # takes half a minute at this size)
        n, rs = 30000, np.random.RandomState(11)
        nnz = int(2e-5 * n * n)
        U = sp.coo_matrix((rs.rand(nnz), (rs.randint(0, n, nnz), rs.randint(0, n, nnz))),
                          shape=(n, n)).tocsr()
        return (sp.eye(n) * 4.0 + sp.triu(U, k=1) - sp.triu(U, k=1).T).tocsr()
    if name == "unsorted_zero_diag":
        A = ml.problems.poisson_2d_5pt(64).tolil()
        A[100, 100] = 0.0  # zero diagonal: that row is skipped
        A = A.tocsr()
        A.sort_indices()
        ip, ij, ax = A.indptr.copy(), A.indices.copy(), A.data.copy()
        for r in range(0, A.shape[0], 3):  # reverse the stored order of every third row
            ij[ip[r]:ip[r + 1]] = ij[ip[r]:ip[r + 1]][::-1].copy()
            ax[ip[r]:ip[r + 1]] = ax[ip[r]:ip[r + 1]][::-1].copy()
        # row 7 stores its diagonal twice (the last one counts)
        ij = np.concatenate([ij[:ip[8]], [7], ij[ip[8]:]]).astype(np.int32)
        ax = np.concatenate([ax[:ip[8]], [5.0], ax[ip[8]:]])
        ip[8:] += 1
        return sp.csr_matrix((ax, ij, ip), shape=A.shape)
    raise KeyError(name)


def _columns_match_single(torch, gs, X0, B, X, iterations):
    """column j of the block result X == GaussSeidel.sweep on a contiguous copy of column j"""
    n, k = X0.shape
    Xh = host(X)
    for j in range(k):
        xj = X0[:, j].clone(memory_format=torch.contiguous_format)  # k = 1: a view otherwise
        bj = (B[:, j].contiguous() if B is not None
              else torch.zeros(n, dtype=torch.float64, device="cuda"))
        gs.sweep(xj, bj, iterations)
        assert np.array_equal(Xh[:, j], host(xj)), (k, j, iterations)


# ---------------------------------------------------------------- 1. the sweep, per path
@pytest.mark.parametrize("name,path", (("grid_60", WALK_PACKED), ("cube_12", WALK_PACKED),
                                       ("long_rows_24", WALK_CSR), ("wide_levels", PER_LEVEL),
                                       ("unsorted_zero_diag", WALK_PACKED)))
def test_sweep_matches_single_sweeps(ml, oracle, torch_cuda, name, path):
    torch = torch_cuda
    A = _matrix(ml, name)
    n = A.shape[0]
    gs = ml.multigrid.GaussSeidel(ml.sparse.DeviceCSR.from_scipy(A, check=False))
    rs = np.random.RandomState(21)
    for k in KS:
        assert gs.mv_path(k) == path, (name, k, gs.mv_path(k), gs.n_levels)
        X0h, Bh = rs.standard_normal((n, k)), rs.standard_normal((n, k))
        X0, B = dev(torch, X0h), dev(torch, Bh)
        for iterations in (1, 3):
            X = X0.clone()
            assert gs.sweep(X, B, iterations) is X
            _columns_match_single(torch, gs, X0, B, X, iterations)
            if name == "grid_60":  # the sequential sweep itself
                Xh = host(X)
                for j in range(k):
                    ref = oracle.gauss_seidel(A, X0h[:, j].copy(), Bh[:, j].copy(),
                                              iterations=iterations)
                    assert np.array_equal(Xh[:, j], ref), (k, j, iterations)


@pytest.mark.parametrize("name,rows,walk,k_walk,k_level",
                         (("grid_300", 300, WALK_PACKED, 26, 28),
                          ("long_rows_240", 80, WALK_CSR, 50, 52)))
def test_sweep_across_the_selection_constants(ml, torch_cuda, name, rows, walk, k_walk, k_level):
    """The widest level of poisson_2d_5pt(300) has 300 rows (an anti-diagonal): k = 26 (13 column
    pairs, 3,900 items) is still walked on the packed copy, k = 28 (14 pairs, 4,200 items) goes
    one launch per level. The widest level of the 25-point matrix at m = 240 has 80 rows (level
    3 i + j of grid point (i, j)): k = 50 (2,000 items) is walked on the CSR arrays, k = 52
    (2,080 items) is not."""
    torch = torch_cuda
    A = ml.problems.poisson_2d_5pt(300).tocsr() if name == "grid_300" else _matrix(ml, name)
    n = A.shape[0]
    gs = ml.multigrid.GaussSeidel(ml.sparse.DeviceCSR.from_scipy(A))
    limit = WALK_ITEMS if walk == WALK_PACKED else WALK_ITEMS_CSR
    assert rows * ((k_walk + 1) // 2) <= limit < rows * ((k_level + 1) // 2)
    rs = np.random.RandomState(22)
    for k, path in ((k_walk, walk), (k_level, PER_LEVEL)):
        assert gs.mv_path(k) == path, (k, gs.mv_path(k))
        X0, B = dev(torch, rs.standard_normal((n, k))), dev(torch, rs.standard_normal((n, k)))
        X = X0.clone()
        gs.sweep(X, B, 1)
        _columns_match_single(torch, gs, X0, B, X, 1)


# ---------------------------------------------------------------- 2. arithmetic x direction
@pytest.mark.parametrize("sweep", ("forward", "backward", "symmetric"))
@pytest.mark.parametrize("block", (False, True))
def test_arithmetic_and_direction(ml, oracle, torch_cuda, block, sweep):
    torch = torch_cuda
    A = ml.problems.poisson_2d_5pt(33).tocsr()
    n, k = A.shape[0], 5
    gs = ml.multigrid.GaussSeidel(ml.sparse.DeviceCSR.from_scipy(A), sweep, block=block)
    rs = np.random.RandomState(23)
    X0h, Bh = rs.standard_normal((n, k)), rs.standard_normal((n, k))
    X0, B = dev(torch, X0h), dev(torch, Bh)
    ref_sweep = oracle.pyamg_block_gauss_seidel if block else oracle.pyamg_gauss_seidel
    for iterations in (1, 2):
        X = X0.clone()
        gs.sweep(X, B, iterations)
        _columns_match_single(torch, gs, X0, B, X, iterations)
        Xh = host(X)
        for j in range(k):
            ref = ref_sweep(A, X0h[:, j].copy(), Bh[:, j].copy(), iterations=iterations,
                            sweep=sweep)
            assert np.array_equal(Xh[:, j], ref), (block, sweep, j, iterations)


# ---------------------------------------------------------------- 3. strides and aliasing
@pytest.mark.parametrize("name", ("grid_60", "long_rows_24", "wide_levels"))
def test_strides_and_zero_rhs(ml, torch_cuda, name):
    torch = torch_cuda
    A = _matrix(ml, name)
    n = A.shape[0]
    gs = ml.multigrid.GaussSeidel(ml.sparse.DeviceCSR.from_scipy(A))
    rs = np.random.RandomState(24)
    for k in (3, 4):
        X0, B = dev(torch, rs.standard_normal((n, k))), dev(torch, rs.standard_normal((n, k)))
        ref = X0.clone()
        gs.sweep(ref, B, 2)  # contiguous: ld = k
        # a column slice at an odd column offset of a wider tensor: 8-byte accesses
        wide = dev(torch, rs.standard_normal((n, k + 4)))
        before = host(wide).copy()
        wide[:, 1:1 + k] = X0
        view = wide[:, 1:1 + k]
        assert view.data_ptr() % 16 == 8
        gs.sweep(view, B, 2)
        after = host(wide)
        assert np.array_equal(after[:, 1:1 + k], host(ref))
        assert np.array_equal(after[:, :1], before[:, :1])
        assert np.array_equal(after[:, 1 + k:], before[:, 1 + k:])
        # 16-byte-aligned blocks with even leading dimensions: 16-byte accesses (k = 3: the last
        # column is a scalar lane)
        wide2 = dev(torch, rs.standard_normal((n, 8)))
        before2 = host(wide2).copy()
        wide2[:, 2:2 + k] = X0
        Bw = dev(torch, rs.standard_normal((n, 6)))
        Bw[:, :k] = B
        assert wide2[:, 2:2 + k].data_ptr() % 16 == 0 and Bw.data_ptr() % 16 == 0
        gs.sweep(wide2[:, 2:2 + k], Bw[:, :k], 2)
        after2 = host(wide2)
        assert np.array_equal(after2[:, 2:2 + k], host(ref))
        assert np.array_equal(after2[:, :2], before2[:, :2])
        assert np.array_equal(after2[:, 2 + k:], before2[:, 2 + k:])
        # b = None equals an all-zero b
        Xn, Xz = X0.clone(), X0.clone()
        gs.sweep(Xn, None, 2)
        gs.sweep(Xz, torch.zeros_like(B), 2)
        assert np.array_equal(host(Xn), host(Xz))
        _columns_match_single(torch, gs, X0, None, Xn, 2)


def test_refused_arguments(ml, torch_cuda):
    torch = torch_cuda
    from mlamg._lib import MLAMG_EINVAL, MlamgError, ptr, stream_ptr
    A = ml.problems.poisson_2d_5pt(12).tocsr()
    n = A.shape[0]
    gs = ml.multigrid.GaussSeidel(ml.sparse.DeviceCSR.from_scipy(A))
    X = torch.ones((n, 4), dtype=torch.float64, device="cuda")
    B = torch.ones((n, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(MlamgError, match="B and X must differ") as ei:
        gs.sweep(X, X, 1)
    assert ei.value.code == MLAMG_EINVAL
    with pytest.raises(ValueError):
        gs.sweep(torch.ones((n, 65), dtype=torch.float64, device="cuda"), None, 1)
    with pytest.raises(ValueError):  # a row stride below the width
        gs.sweep(torch.as_strided(X, (n, 4), (3, 1)), B, 1)
    with pytest.raises(ValueError):
        gs.sweep(X, B[:, :3], 1)
    with pytest.raises(ValueError):
        gs.mv_path(65)
    s = stream_ptr()
    for args, word in (((ptr(X), 4, ptr(B), 4, 65, 1, s), "k must be in"),
                       ((ptr(X), 3, ptr(B), 4, 4, 1, s), "ldx < k"),
                       ((ptr(X), 4, ptr(B), 3, 4, 1, s), "ldb < k"),
                       ((None, 4, ptr(B), 4, 4, 1, s), "X is NULL")):
        with pytest.raises(MlamgError, match=word) as ei:
            _call("mlamg_gs_sweep_mv", gs.handle, *args)
        assert ei.value.code == MLAMG_EINVAL
    assert np.all(host(X) == 1.0)


# ---------------------------------------------------------------- 4, 5. the block cycle
def _sa_P(A, agg, omega=2.0 / 3.0):
    """P = (I - omega D^-1 A) Agg (ns/lib/multigrid.py:102-108) in scipy."""
    n = A.shape[0]
    Dinv = sp.diags([1.0 / A.diagonal()], [0])
    return sp.csr_matrix((sp.eye(n) - omega * Dinv @ A) @ agg)


def _agg_matrix(ml, m, size=3):
    agg = ml.problems.box_aggregates_2d(m, m, size)
    if sp.issparse(agg):
        return sp.csr_matrix(agg)
    lab = np.asarray(agg).ravel()
    return sp.csr_matrix((np.ones(lab.size), (np.arange(lab.size), lab)))


def _single_loop(torch, H, b, x, n_cycles, norm, remove_mean):
    """n_cycles single-vector cycles on (b, x), each followed by the mean removal (if asked)
    and mlamg_norm2 of the freshly computed residual (or of x): the history cycle_multi is
    defined by (tests/test_gpu_multivector.py)."""
    from mlamg._lib import ptr, stream_ptr
    A = H.levels[0].A
    n = x.numel()
    s = stream_ptr()
    bz = b if b is not None else torch.zeros(n, dtype=torch.float64, device="cuda")
    hist = []
    for _ in range(n_cycles):
        H.cycle(bz, x, 1, use_graph=False, history=False)
        if remove_mean:
            _call("mlamg_remove_mean", ptr(x), n, s)
        v = x
        if norm == "residual":
            v = torch.empty(n, dtype=torch.float64, device="cuda")
            _call("mlamg_residual", A.handle, ptr(bz), ptr(x), ptr(v), None, s)
        nj = torch.empty(1, dtype=torch.float64, device="cuda")
        _call("mlamg_norm2", ptr(v), n, ptr(nj), s)
        hist.append(host(nj)[0])
    return np.array(hist)


@pytest.fixture(scope="module")
def two_level_gs(ml, torch_cuda):
    A = ml.problems.poisson_2d_5pt(32).tocsr()
    return ml.hierarchy.Hierarchy.two_level(A, _sa_P(A, _agg_matrix(ml, 32)),
                                            smoother="gauss_seidel")


@pytest.mark.parametrize("nu", ((1, 1), (2, 1), (0, 1)))
def test_two_level_cycle_matches_single_cycles(ml, torch_cuda, two_level_gs, nu):
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    H = two_level_gs
    assert H.enable_block_gauss_seidel() is H
    _call("mlamg_hier_set_smoothing", H.handle, nu[0], nu[1])
    n = H.levels[0].A.shape[0]
    k, cycles = 6, 4
    rs = np.random.RandomState(7)
    X0 = dev(torch, rs.standard_normal((n, k)))
    B = dev(torch, rs.standard_normal((n, k)))
    try:
        for norm, remove_mean, Bm in (("residual", False, B), ("x", True, B),
                                      ("residual", True, None), ("x", False, None)):
            X = X0.clone()
            hist = H.cycle_multi(Bm, X, cycles, norm=norm, remove_mean=remove_mean)
            assert hist.shape == (cycles, k)
            X2 = X0.clone()
            hist2 = H.cycle_multi(Bm, X2, cycles, norm=norm, remove_mean=remove_mean)
            assert np.array_equal(host(X), host(X2)) and np.array_equal(hist, hist2)
            for j in range(k):
                xj = X0[:, j].contiguous()
                bj = Bm[:, j].contiguous() if Bm is not None else None
                hj = _single_loop(torch, H, bj, xj, cycles, norm, remove_mean)
                assert np.array_equal(host(X[:, j]), host(xj)), (norm, remove_mean, j)
                assert np.array_equal(hist[:, j], hj), (norm, remove_mean, j, hist[:, j], hj)
        # the switch off again: the documented refusal, word for word
        H.enable_block_gauss_seidel(False)
        with pytest.raises(MlamgError, match=r"a level uses a Gauss-Seidel smoother "
                                             r"\(weighted Jacobi only\)") as ei:
            H.cycle_multi(B, X0.clone(), 1)
        assert ei.value.code == MLAMG_EUNSUPPORTED
    finally:
        H.enable_block_gauss_seidel(False)
        _call("mlamg_hier_set_smoothing", H.handle, 1, 1)


def test_multilevel_pyamg_sa_cycle(ml, torch_cuda):
    """pyamg_sa: symmetric block Gauss-Seidel on every level, pinv coarse product."""
    torch = torch_cuda
    from mlamg._lib import MlamgError
    H = ml.hierarchy.Hierarchy.pyamg_sa(ml.problems.poisson_2d_5pt(48))
    assert H.n_levels >= 3
    n, k = H.levels[0].A.shape[0], 5
    rs = np.random.RandomState(9)
    B = dev(torch, rs.standard_normal((n, k)))
    with pytest.raises(MlamgError, match="Gauss-Seidel"):
        H.precondition(B)
    H.enable_block_gauss_seidel()
    Z = H.precondition(B)
    assert tuple(Z.shape) == (n, k)
    for j in range(k):
        zj = H.precondition(B[:, j].contiguous())
        assert np.array_equal(host(Z[:, j]), host(zj)), j
    X0 = dev(torch, rs.standard_normal((n, k)))
    X = X0.clone()
    hist = H.cycle_multi(B, X, 3)
    for j in range(k):
        xj = X0[:, j].contiguous()
        hj = _single_loop(torch, H, B[:, j].contiguous(), xj, 3, "residual", False)
        assert np.array_equal(host(X[:, j]), host(xj)), j
        assert np.array_equal(hist[:, j], hj), (j, hist[:, j], hj)
