"""GPU parity: every hot-path kernel through the C-ABI against the reference golden vectors and
the oracle. Bitwise for SpMV / residual / Jacobi / restriction / prolongation / SpGEMM /
Galerkin / aggregation; fp64 tolerances (stated per test) for eigenvalues, coarse solves, norms."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import gs_cases
from conftest import golden_csr

pytestmark = pytest.mark.gpu

MATS = ("c1", "p2d", "lap3d", "rnd")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.graph
    import mlamg.hierarchy
    import mlamg.multigrid
    import mlamg.sparse
    import mlamg.strength
    return mlamg


def dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- SpMV family
@pytest.mark.parametrize("k", MATS)
def test_spmv_residual_bitwise(golden, ml, torch_cuda, k):
    torch = torch_cuda
    A = golden_csr(golden, k)
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    x, b = dev(torch, golden[f"{k}_x"]), dev(torch, golden[f"{k}_b"])
    y = Ad.matvec(x)
    assert np.array_equal(host(y), golden[f"{k}_Ax"])
    r = torch.empty_like(b)
    nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
    from mlamg._lib import call, ptr, stream_ptr
    call("mlamg_residual", Ad.handle, ptr(b), ptr(x), ptr(r), ptr(nrm), stream_ptr())
    assert np.array_equal(host(r), golden[f"{k}_resid"])
    ref = np.linalg.norm(golden[f"{k}_resid"])
    assert abs(nrm.item() - ref) <= 1e-13 * ref  # reduction order differs from BLAS dnrm2/dot


@pytest.mark.parametrize("k", MATS)
@pytest.mark.parametrize("nu", (1, 2, 5))
def test_multigrid_jacobi_bitwise(golden, ml, k, nu):
    A = golden_csr(golden, k)
    x = golden[f"{k}_x"].copy()
    out = ml.multigrid.jacobi(A, golden[f"{k}_b"], x, omega=0.666, nu=nu)
    assert out is x
    assert np.array_equal(x, golden[f"{k}_jacobi_nu{nu}"])


@pytest.mark.parametrize("k", MATS)
def test_mlamg_jacobi_bitwise(golden, ml, oracle, torch_cuda, k):
    torch = torch_cuda
    A = golden_csr(golden, k)
    Dw = oracle.mlamg_dinv(A)
    ref = oracle.jacobi_mlamg(A, Dw, golden[f"{k}_b"], golden[f"{k}_x"].copy(), nu=3)
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    dw = Ad.diag_inv(2.0 / 3.0)
    assert np.array_equal(host(dw), Dw.diagonal())
    x = dev(torch, golden[f"{k}_x"])
    tmp = torch.empty_like(x)
    from mlamg._lib import call, ptr, stream_ptr
    bd = dev(torch, golden[f"{k}_b"])
    call("mlamg_jacobi", Ad.handle, ptr(dw), ptr(bd), ptr(x), ptr(tmp),
         3, stream_ptr())
    assert np.array_equal(host(x), ref)


def test_restrict_prolong_transpose_bitwise(golden, ml, torch_cuda):
    torch = torch_cuda
    A = golden_csr(golden, "c1")
    P = sp.csr_matrix((golden["c1_P_data"], golden["c1_P_indices"], golden["c1_P_indptr"]),
                      shape=(1024, 342))
    Pd = ml.sparse.DeviceCSR.from_scipy(P)
    Rd = Pd.transpose()
    R = Rd.to_scipy()
    Rref = P.T.tocsr()
    assert np.array_equal(R.indptr, Rref.indptr) and np.array_equal(R.indices, Rref.indices)
    assert np.array_equal(R.data, Rref.data)
    r = np.random.RandomState(5).randn(1024)
    rc = torch.empty(342, dtype=torch.float64, device="cuda")
    from mlamg._lib import call, ptr, stream_ptr
    rd = dev(torch, r)
    call("mlamg_restrict", Rd.handle, ptr(rd), ptr(rc), stream_ptr())
    assert np.array_equal(host(rc), P.T @ r)  # scipy csc_matvec
    e = np.random.RandomState(6).randn(342)
    x = np.random.RandomState(7).randn(1024)
    xd = dev(torch, x)
    ed = dev(torch, e)
    call("mlamg_prolong_add", Pd.handle, ptr(ed), ptr(xd), stream_ptr())
    xr = x.copy()
    xr += P @ e
    assert np.array_equal(host(xd), xr)


# ---------------------------------------------------------------- setup kernels
def test_sa_prolongator_galerkin_bitwise(golden, ml):
    A = golden_csr(golden, "c1")
    Agg = sp.csr_matrix((np.ones(1024), golden["c1_Agg_indices"], golden["c1_Agg_indptr"]),
                        shape=(1024, 342))
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    Aggd = ml.sparse.DeviceCSR.from_scipy(Agg)
    Pd, om = ml.multigrid.smoothed_aggregation_jacobi_device(Ad, Aggd, float(golden["c1_omega"]))
    P = Pd.to_scipy()
    assert np.array_equal(P.indptr, golden["c1_P_indptr"])
    assert np.array_equal(P.indices, golden["c1_P_indices"])  # scipy's stored column order too
    assert np.array_equal(P.data, golden["c1_P_data"])
    AH = ml.sparse.galerkin(Pd.transpose(), Ad, Pd).to_scipy()
    assert np.array_equal(AH.indptr, golden["c1_AH_indptr"])
    assert np.array_equal(AH.indices, golden["c1_AH_indices"])
    assert np.array_equal(AH.data, golden["c1_AH_data"])


@pytest.fixture(params=("esc", "dense"))
def spgemm_path(request, monkeypatch):
    """Run with each SpGEMM algorithm (expand-sort-compress / dense LDS rows)."""
    monkeypatch.setenv("MLAMG_SPGEMM", request.param)
    return request.param


@pytest.mark.parametrize("seed", (0, 1))
def test_galerkin_random_bitwise(ml, seed, spgemm_path):
    """(P^T A) P on the device vs scipy's P.T @ A @ P (CSC path), values bit for bit, including
    cancellations (exact zeros dropped) and rows with no products."""
    rs = np.random.RandomState(seed)
    n, nc = 4000, 500
    A = sp.random(n, n, density=0.003, random_state=rs, format="csr") + sp.eye(n, format="csr")
    A = A.tocsr()
    A.sort_indices()
    A.data[::5] *= -1
    agg = rs.randint(0, nc, n)
    agg[:7] = nc - 1  # some coarse columns empty, others heavy
    T = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, nc))
    P = (T + sp.random(n, nc, density=0.002, random_state=rs, format="csr")).tocsr()
    P.sort_indices()
    P.data[::3] = np.round(P.data[::3] * 4) / 4  # small dyadic values make exact cancellations
    ref = (P.T @ A @ P).tocsr()
    ref.sort_indices()
    ref.eliminate_zeros()
    Ad, Pd = ml.sparse.DeviceCSR.from_scipy(A), ml.sparse.DeviceCSR.from_scipy(P)
    AH = ml.sparse.galerkin(Pd.transpose(), Ad, Pd).to_scipy()
    assert np.array_equal(AH.indptr, ref.indptr)
    assert np.array_equal(AH.indices, ref.indices)
    assert np.array_equal(AH.data, ref.data)


@pytest.mark.parametrize("k", ("c1", "p2d", "lap3d", "rnd"))
def test_lambda_max_vs_arpack(golden, ml, oracle, k):
    A = golden_csr(golden, k)
    lam, its = ml.multigrid.lambda_max_dinv_a(A)
    ref = oracle.arpack_lambda_max(A)
    assert abs(lam - ref) <= 1e-12 * ref, (lam, ref, its)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_spgemm_scipy_layout_random(ml, seed):
    rs = np.random.RandomState(seed)
    A = sp.random(300, 200, density=0.05, random_state=rs, format="csr")
    B = sp.random(200, 250, density=0.05, random_state=rs, format="csr")
    B.data[::7] *= -1
    C = (A @ B)  # scipy csr_matmat: unsorted columns, exact zeros dropped
    Cd = (ml.sparse.DeviceCSR.from_scipy(A) @ ml.sparse.DeviceCSR.from_scipy(B)).to_scipy()
    assert np.array_equal(Cd.indptr, C.indptr)
    assert np.array_equal(Cd.indices, C.indices)
    assert np.array_equal(Cd.data, C.data)


def test_spgemm_drops_exact_zeros(ml):
    A = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, -1.0]]))
    B = sp.csr_matrix(np.array([[1.0, 2.0], [-1.0, 2.0]]))
    C = A @ B  # [[1-1, 2+2], [1+1, 2-2]]: two entries cancel exactly and are dropped
    Cd = (ml.sparse.DeviceCSR.from_scipy(A) @ ml.sparse.DeviceCSR.from_scipy(B)).to_scipy()
    assert C.nnz == Cd.nnz == 2
    assert np.array_equal(Cd.toarray(), C.toarray())


def test_empty_and_ragged(ml, torch_cuda):
    torch = torch_cuda
    # rows of length 0, 1 and one row longer than an LDS chunk (2048)
    n = 3000
    rows = [np.array([], int), np.array([5]), np.arange(n)]
    indptr = np.cumsum([0] + [len(r) for r in rows] + [1] * (n - 3))
    indices = np.concatenate(rows + [np.arange(3, n)])
    data = np.random.RandomState(0).randn(len(indices))
    A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    x = np.random.RandomState(1).randn(n)
    y = host(ml.sparse.DeviceCSR.from_scipy(A).matvec(dev(torch, x)))
    assert np.array_equal(y, A @ x)
    E = sp.csr_matrix((0, 0))
    Ed = ml.sparse.DeviceCSR.from_scipy(E)
    assert Ed.shape == (0, 0)


# ---------------------------------------------------------------- aggregation
CALLERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "reference_callers.npz")


@pytest.fixture(scope="module")
def callers():
    return dict(np.load(CALLERS, allow_pickle=False))


def _weights(A, kind):
    if kind == "invabs":
        return sp.csr_matrix((1.0 / np.abs(A.data), A.indices, A.indptr), A.shape)
    return sp.csr_matrix((np.ones_like(A.data), A.indices, A.indptr), A.shape)


@pytest.mark.parametrize("k", ("p2d", "rnd", "lap3d"))
def test_bellman_ford(golden, ml, oracle, k):
    """modified_bellman_ford (ns/lib/graph.py:7-53): distances AND nearest centers bitwise the
    reference's own outputs (tests/golden/reference_vectors.npz) — the constant-coefficient p2d
    and lap3d graphs are tie-rich."""
    import torch
    A = golden_csr(golden, k)
    C = _weights(A, "invabs")
    seeds = golden[f"{k}_bf_seeds"]
    S_T = ml.sparse.to_torch_sparse(C)
    d, nc = ml.graph.modified_bellman_ford(S_T, torch.as_tensor(seeds))
    assert d.dtype == torch.float32 and nc.dtype == torch.int64
    assert np.array_equal(d.numpy(), golden[f"{k}_bf_dist"])
    assert np.array_equal(nc.numpy(), golden[f"{k}_bf_nearest"])


@pytest.mark.parametrize("k", ("p2d", "rnd", "lap3d"))
@pytest.mark.parametrize("seed", (1, 5))
def test_bellman_ford_unit_weights(golden, ml, oracle, k, seed):
    """Unit weights (every path length an integer: ties everywhere) and other seed draws,
    against the oracle's transcription of the reference sweep (itself bitwise the reference on
    the goldens above, tests/test_oracle_golden.py); the reference's sweep count as well."""
    import torch
    from mlamg.sparse import DeviceCSR
    A = golden_csr(golden, k)
    C = _weights(A, "unit")
    n = A.shape[0]
    seeds = np.random.RandomState(seed).permutation(n)[:int(np.ceil(0.07 * n))]
    dr, zr, swr = oracle.modified_bellman_ford(C, seeds)
    d, nc = ml.graph.modified_bellman_ford(ml.sparse.to_torch_sparse(C), torch.as_tensor(seeds))
    assert np.array_equal(d.numpy(), dr) and np.array_equal(nc.numpy(), zr)
    sd = torch.as_tensor(seeds.astype(np.int32)).cuda()
    _, _, sw = ml.graph.modified_bellman_ford_device(DeviceCSR.from_scipy(C), sd)
    assert sw == swr


@pytest.mark.parametrize("k", ("p2d", "rnd", "lap3d"))
def test_bellman_ford_canon(golden, ml, oracle, k):
    """The hierarchy's order-independent variant (mlamg_bellman_ford_canon): same distances,
    labels = the oracle's restatement of its rule; = the reference's labels on tie-free rnd."""
    import torch
    from mlamg.sparse import DeviceCSR
    A = golden_csr(golden, k)
    C = _weights(A, "invabs")
    seeds = golden[f"{k}_bf_seeds"]
    d, lab, _ = ml.graph.bellman_ford_device(
        DeviceCSR.from_scipy(C), torch.as_tensor(seeds.astype(np.int32)).cuda())
    dc, labc = oracle.canon_bellman_ford(C, seeds)
    assert np.array_equal(d.cpu().numpy(), golden[f"{k}_bf_dist"])
    assert np.array_equal(lab.cpu().numpy(), labc)
    agree = float(np.mean(np.where(labc < 0, 0, labc) == golden[f"{k}_bf_nearest"]))
    if k == "rnd":
        assert agree == 1.0


def test_bellman_ford_wide_graph(ml, oracle):
    """Graphs above 2^18 nodes take the per-level launches (graph.hip kSeqOneBlockMax): the
    push sweep and pyamg's pull sweep bitwise against the oracle on a 520^2 unit-weight grid."""
    import torch
    from mlamg import problems
    from mlamg.sparse import DeviceCSR
    A = problems.poisson_2d_5pt(520)
    C = _weights(A, "unit")
    n = A.shape[0]
    seeds = np.random.RandomState(0).permutation(n)[:int(np.ceil(0.1 * n))]
    dr, zr, swr = oracle.modified_bellman_ford(C, seeds)
    sd = torch.as_tensor(seeds.astype(np.int32)).cuda()
    Cd = DeviceCSR.from_scipy(C)
    d, z, sw = ml.graph.modified_bellman_ford_device(Cd, sd)
    zd = z.cpu().numpy().astype(np.int64)
    assert np.array_equal(d.cpu().numpy(), dr)
    assert np.array_equal(np.where(zd < 0, 0, zd), zr) and sw == swr
    dp, zp, swp = oracle.pyamg_bellman_ford(C, seeds)
    d2, z2, sw2 = ml.graph.bellman_ford_pyamg_device(Cd, sd)
    assert np.array_equal(d2.cpu().numpy(), dp) and np.array_equal(z2.cpu().numpy(), zp)
    assert sw2 == swp
    Cs = C.copy()
    dl, cl, sl = oracle.lloyd_cluster(Cs, seeds[:2000].copy(), maxiter=3, canon=False)
    d3, c3, s3, _ = ml.graph.lloyd_cluster_device(Cd, sd[:2000].clone(), maxiter=3)
    assert np.array_equal(c3.cpu().numpy(), cl) and np.array_equal(s3.cpu().numpy(), sl)
    assert np.array_equal(d3.cpu().numpy(), dl)


@pytest.mark.parametrize("k", ("p2d", "rnd", "lap3d"))
def test_nearest_center_to_agg(golden, ml, k):
    import torch
    seeds = torch.as_tensor(golden[f"{k}_bf_seeds"])
    T = ml.graph.nearest_center_to_agg(seeds, torch.as_tensor(golden[f"{k}_bf_nearest"]))
    assert np.array_equal(T.indices().numpy(), golden[f"{k}_agg_idx"])
    assert T.dtype == torch.float32
    with pytest.raises(KeyError):
        ml.graph.nearest_center_to_agg(seeds[:3], torch.as_tensor(golden[f"{k}_bf_nearest"]))


def test_lloyd_aggregation(golden, ml, oracle):
    A = golden_csr(golden, "rnd")
    C = sp.csr_matrix((1.0 / np.abs(A.data), A.indices, A.indptr), A.shape)
    AggOp, roots, seeds = ml.graph.lloyd_aggregation(C, ratio=0.1, distance='same', rand=0)
    assert np.array_equal(seeds, golden["rnd_lloyd_seeds"])
    assert np.array_equal(roots, golden["rnd_lloyd_roots"])
    assert np.array_equal(AggOp.indptr, golden["rnd_lloyd_agg_indptr"])
    assert np.array_equal(AggOp.indices, golden["rnd_lloyd_agg_indices"])
    assert AggOp.dtype == np.int8


@pytest.mark.parametrize("k", ("p2d", "lap3d"))
@pytest.mark.parametrize("case", ("unit0", "unit3", "olson"))
def test_lloyd_tie_rich_matches_reference(golden, callers, ml, oracle, k, case):
    """ns.lib.graph.lloyd_aggregation on tie-rich graphs — 'unit' distances (rand 0, 3) and the
    evaluation loops' default path (np.random.seed(0), olson measure, 'same', rand=0,
    utils/common.py:51-58) — against the reference driver's output with the ORACLE's
    pyamg-order lloyd_cluster standing in for pyamg (tests/golden/reference_callers.npz): seeds,
    roots and AggOp bitwise. A SELF-CONSISTENCY check of the cluster kernel against its
    restatement inside the reference driver (seeding, distance transform, AggOp assembly are
    the reference's own code); parity with pyamg's amg_core tie-breaking is unpinned (absent)."""
    A = golden_csr(golden, k)
    if case == "olson":
        np.random.seed(0)
        C = ml.strength.strength_measure_funcs["olson"](A)
        AggOp, roots, seeds = ml.graph.lloyd_aggregation(C, ratio=0.1, distance='same', rand=0)
    else:
        C = _weights(A, "unit")
        AggOp, roots, seeds = ml.graph.lloyd_aggregation(C, ratio=0.1, distance='unit',
                                                         rand=int(case[-1]))
    assert np.array_equal(seeds, callers[f"{k}_{case}_seeds"])
    assert np.array_equal(roots, callers[f"{k}_{case}_roots"])
    assert np.array_equal(AggOp.indptr, callers[f"{k}_{case}_agg_indptr"])
    assert np.array_equal(AggOp.indices, callers[f"{k}_{case}_agg_indices"])


@pytest.mark.parametrize("k", ("p2d", "lap3d"))
@pytest.mark.parametrize("rand", (1, 7))
@pytest.mark.parametrize("distance", ("unit", "abs"))
def test_lloyd_tie_rich_matches_oracle(golden, ml, oracle, k, rand, distance):
    """More tie-rich draws against the oracle's pyamg-order restatement (canon=False), and the
    hierarchy's order-independent variant against the oracle's restatement of its rule."""
    from mlamg.sparse import DeviceCSR
    import torch
    A = golden_csr(golden, k)
    C = abs(A).tocsr()
    AggOp, roots, _ = ml.graph.lloyd_aggregation(C, ratio=0.1, distance=distance, rand=rand)
    AggR, rootsR, _ = oracle.lloyd_aggregation(C, ratio=0.1, distance=distance, rand=rand)
    assert np.array_equal(roots, rootsR)
    assert np.array_equal(AggOp.indices, AggR.indices)
    G = ml.graph.distance_data(C, distance)
    G = sp.csr_matrix((G, C.indices, C.indptr), shape=C.shape)
    seeds = np.random.RandomState(rand).permutation(A.shape[0])[:int(np.ceil(0.1 * A.shape[0]))]
    _, cc, sc = oracle.lloyd_cluster(G, seeds.copy(), maxiter=10, canon=True)
    _, c, s, _ = ml.graph.lloyd_cluster_device(DeviceCSR.from_scipy(G),
                                               torch.as_tensor(seeds.astype(np.int32)).cuda(),
                                               10, exact=False)
    assert np.array_equal(c.cpu().numpy(), cc) and np.array_equal(s.cpu().numpy(), sc)


# ---------------------------------------------------------------- smoothers / coarse solve
@pytest.mark.parametrize("k", MATS)
def test_gauss_seidel_bitwise(golden, ml, oracle, k):
    A = golden_csr(golden, k)
    x = golden[f"{k}_x"].copy()
    ref = oracle.gauss_seidel(A, x.copy(), golden[f"{k}_b"], iterations=2)
    got = ml.multigrid.gauss_seidel(A, golden[f"{k}_b"], x, nu=2)
    assert np.array_equal(got, ref)


def test_dense_coarse_solve(golden, ml, torch_cuda):
    torch = torch_cuda
    AH = sp.csr_matrix((golden["c1_AH_data"], golden["c1_AH_indices"], golden["c1_AH_indptr"]))
    b = np.random.RandomState(3).randn(AH.shape[0])
    import ctypes
    from mlamg._lib import call, ptr, stream_ptr
    Ad = ml.sparse.DeviceCSR.from_scipy(AH)
    h = ctypes.c_void_p()
    call("mlamg_dense_create", Ad.handle, ctypes.byref(h), stream_ptr())
    x = torch.empty(AH.shape[0], dtype=torch.float64, device="cuda")
    bd = dev(torch, b)
    call("mlamg_dense_solve", h, ptr(bd), ptr(x), stream_ptr())
    ref = np.linalg.solve(AH.toarray(), b)
    call("mlamg_dense_destroy", h)
    assert np.allclose(host(x), ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("n", (64, 97, 300, 1025, 2100))
def test_dense_inverse_cholesky(ml, torch_cuda, n):
    """Symmetric positive definite coarse operators take the device-wide inverse Cholesky
    factor (dense.hip: 32-column panels, MFMA trailing updates, A^-1 = X^T X, or from 2048 rows
    the factor kept and applied as X^T (X b)); an unsymmetric one takes Gauss-Jordan. Both
    against numpy's inverse at fp64 tolerance (sizes straddle the panel and tile edges)."""
    torch = torch_cuda
    import ctypes
    from mlamg._lib import call, ptr, stream_ptr
    rs = np.random.RandomState(n)
    B = sp.random(n, n, density=min(1.0, 12.0 / n), random_state=rs, format="csr")
    S = (B + B.T).tocsr()
    A = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()  # SPD (diag. dom.)
    for M, method in ((A, 1 if n < 2048 else 2), ((A + sp.triu(B, 1) * 0.5).tocsr(), 0)):
        Md = ml.sparse.DeviceCSR.from_scipy(M)
        h = ctypes.c_void_p()
        call("mlamg_dense_create", Md.handle, ctypes.byref(h), stream_ptr())
        meth = ctypes.c_int()
        call("mlamg_dense_info", h, ctypes.byref(meth), None)
        assert meth.value == method
        b = rs.randn(n)
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        call("mlamg_dense_solve", h, ptr(dev(torch, b)), ptr(x), stream_ptr())
        call("mlamg_dense_destroy", h)
        ref = np.linalg.solve(M.toarray(), b)
        assert np.allclose(host(x), ref, rtol=1e-11, atol=1e-12 * np.abs(ref).max())


def test_two_level_large_coarse_histories(oracle, ml):
    """Two-level amg_2_v at 96^2 (n_c = 1024, the hierarchy engine's dense coarse solve via
    the inverse Cholesky factor) against the oracle's SuperLU-based histories."""
    m = 96
    A = ml.problems.poisson_2d_5pt(m)
    P, _ = oracle.smoothed_aggregation_jacobi(A, ml.problems.box_aggregates_2d(m, m, 3),
                                              omega=2.0 / 3.0)
    x0 = np.random.RandomState(4).randn(A.shape[0])
    b = np.zeros(A.shape[0])
    xr, cr, er, ir = oracle.amg_2_v(A, P, b, x0, res_tol=1e-10)
    x, c, e, it = ml.multigrid.amg_2_v(A, P, b, x0, res_tol=1e-10, engine="hierarchy")
    assert it == ir and np.allclose(e, er, rtol=1e-10, atol=0) and abs(c - cr) <= 1e-8


def test_dense_singular_reported(ml):
    import ctypes
    from mlamg._lib import MlamgError, call, stream_ptr
    Z = ml.sparse.DeviceCSR.from_scipy(sp.csr_matrix(np.array([[1.0, 2.0], [2.0, 4.0]])))
    h = ctypes.c_void_p()
    with pytest.raises(MlamgError, match="singular"):
        call("mlamg_dense_create", Z.handle, ctypes.byref(h), stream_ptr())


# ---------------------------------------------------------------- drivers
def _P1(golden):
    return sp.csr_matrix((golden["c1_P_data"], golden["c1_P_indices"], golden["c1_P_indptr"]),
                         shape=(1024, 342))


@pytest.mark.parametrize("case", ("wide_levels", "grid_200", "grid_1100", "cube_24",
                                  "long_rows", "unsorted_zero_diag", "grid_60_lds", "cube_12_lds",
                                  "grid_256", "nine_point_48", "grid_160", "grid_400",
                                  "nine_point_300"))
def test_gauss_seidel_both_schedules(ml, oracle, torch_cuda, case):
    """Level-scheduled GS through four of its eight paths, each asserted (gs.path against
    gs_cases.BOTH_SCHEDULES, the table the host planner's test checks on the CPU): the per-level
    launches (LEVELS: wide_levels, a level wider than 8192 rows), the pipelined one-workgroup
    kernel with two rows per thread (PIPE: grid_1100, anti-diagonal levels of up to 1100 rows),
    the long-row ring sweep (WRING: long_rows, 25 entries a row) and the windowed sweep (WINDOW,
    levels of <= 512 rows with <= 8 off-diagonals on 1-4 sweeping waves: grid_60, cube_12,
    nine_point_48 whose couplings span 2 levels and the unsorted / zero-diagonal case on one,
    nine_point_300 on 3 with 8 slots per row, grid_160 on 3, grid_200, grid_256 and cube_24 on
    4, grid_400 on 4 with 2 rows per lane; the "_lds" cases are small enough for k_gs_lds but
    take the window, which comes first). The other four paths: test_gauss_seidel_every_path.
    Bitwise the sequential pyamg sweep, including rows stored in non-ascending order, a zero
    diagonal (row left unchanged) and a duplicated diagonal entry; three sweeps per launch."""
    rs = np.random.RandomState(11)
    if case == "wide_levels":
        n = 30000  # diagonal + a sparse upper band: a few levels of ~10^4 independent rows
        U = sp.random(n, n, density=2e-5, random_state=rs, format="csr")
        A = (sp.eye(n) * 4.0 + sp.triu(U, k=1) - sp.triu(U, k=1).T).tocsr()
    elif case == "grid_200":
        A = ml.problems.poisson_2d_5pt(200)
    elif case == "grid_1100":  # anti-diagonal levels of up to 1100 rows
        A = ml.problems.poisson_2d_5pt(1100)
    elif case == "cube_24":
        A = ml.problems.poisson_3d_7pt(24)
    elif case == "grid_256":
        A = ml.problems.poisson_2d_5pt(256)
    elif case in ("grid_160", "grid_400"):
        A = ml.problems.poisson_2d_5pt(int(case[5:]))
    elif case in ("nine_point_48", "nine_point_300"):
        m = int(case[11:])
        T = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(m, m))
        A = (sp.kron(T, T) * -1.0 + sp.eye(m * m) * 9.0).tocsr()
    elif case == "grid_60_lds":  # n <= 8192: x held in LDS for the whole sweep
        A = ml.problems.poisson_2d_5pt(60)
    elif case == "cube_12_lds":
        A = ml.problems.poisson_3d_7pt(12)
    elif case == "long_rows":  # 9-point-like rows with up to 12 off-diagonals
        m = 60
        T = sp.diags([1.0, 1.0, 1.0, 1.0, 1.0], [-2, -1, 0, 1, 2], shape=(m, m))
        A = (sp.kron(T, T) * -0.1 + sp.eye(m * m) * 4.0).tocsr()
    else:
        A = ml.problems.poisson_2d_5pt(64).tolil()
        A[100, 100] = 0.0  # zero diagonal: that row is skipped
        A = A.tocsr()
        A.sort_indices()
        ip, ij, ax = A.indptr.copy(), A.indices.copy(), A.data.copy()
        for r in range(0, A.shape[0], 3):  # reverse the stored order of every third row
            ij[ip[r]:ip[r + 1]] = ij[ip[r]:ip[r + 1]][::-1].copy()
            ax[ip[r]:ip[r + 1]] = ax[ip[r]:ip[r + 1]][::-1].copy()
        # row 7 stores its diagonal twice (the last one counts)
        r7 = slice(ip[7], ip[8])
        ij7, ax7 = list(ij[r7]), list(ax[r7])
        ij = np.concatenate([ij[:ip[8]], [7], ij[ip[8]:]]).astype(np.int32)
        ax = np.concatenate([ax[:ip[8]], [5.0], ax[ip[8]:]])
        ip = ip.copy()
        ip[8:] += 1
        A = sp.csr_matrix((ax, ij, ip), shape=A.shape)
    if case not in ("unsorted_zero_diag",):
        A.sort_indices()
    b = rs.randn(A.shape[0])
    x0 = rs.randn(A.shape[0])
    # stored rows as they are (duplicates included: pyamg takes the last diagonal entry)
    gs = ml.multigrid.GaussSeidel(ml.sparse.DeviceCSR.from_scipy(A, check=False))
    assert gs.PATHS[gs.path] == gs_cases.PATH_NAMES[gs_cases.BOTH_SCHEDULES[case][1]], case
    ref = oracle.gauss_seidel(A, x0.copy(), b, iterations=3)
    xd = torch_cuda.as_tensor(x0.copy()).cuda()
    gs.sweep(xd, torch_cuda.as_tensor(b).cuda(), 3)
    got = xd.cpu().numpy()
    assert np.array_equal(got, ref), (case, gs.n_levels)
    if case != "unsorted_zero_diag":  # the reference-facing entry point
        assert np.array_equal(ml.multigrid.gauss_seidel(A, b, x0.copy(), nu=3), ref)


@pytest.mark.parametrize("case", sorted(gs_cases.EVERY_PATH))
def test_gauss_seidel_every_path(ml, oracle, torch_cuda, monkeypatch, case):
    """The paths test_gauss_seidel_both_schedules does not reach (RING, PIPE_LDS with 4 and 8
    slots, PIPE with one row per thread and 4 and 8 slots, PIPE with two on the 9,000-row slab,
    WAVE and WORKGROUP with and without a knob), each also on the unsorted / zero-diagonal /
    duplicate-diagonal matrix where it takes packed rows: the path asserted (both halves of a
    symmetric handle), then three sweeps bitwise the sequential one, in both arithmetics and
    all three directions. Knobs (MLAMG_GS_NO_*) are read when the handle is created."""
    build, knobs, path = gs_cases.EVERY_PATH[case]
    for k in knobs:
        monkeypatch.setenv("MLAMG_GS_" + k, "1")
    A = build()
    rs = np.random.RandomState(12)
    b, x0 = rs.randn(A.shape[0]), rs.randn(A.shape[0])
    Ad = ml.sparse.DeviceCSR.from_scipy(A, check=False)
    bd = torch_cuda.as_tensor(b).cuda()
    for block in (False, True):
        for sweep in ("forward", "backward", "symmetric"):
            gs = ml.multigrid.GaussSeidel(Ad, sweep, block=block)
            assert gs.PATHS[gs.path] == gs_cases.PATH_NAMES[path], (case, sweep, block)
            if sweep == "symmetric":
                assert gs.PATHS[gs.path_backward] == gs_cases.PATH_NAMES[path], (case, block)
            xd = torch_cuda.as_tensor(x0.copy()).cuda()
            gs.sweep(xd, bd, 3)
            ref = x0.copy()
            if block:
                oracle.pyamg_block_gauss_seidel(A, ref, b, 3, sweep)
            elif sweep == "forward":
                oracle.gauss_seidel(A, ref, b, 3)
            else:
                oracle.pyamg_gauss_seidel(A, ref, b, 3, sweep)
            got = xd.cpu().numpy()
            assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (case, sweep, block)


def test_amg_2_v_gauss_seidel(golden, ml):
    A, P = golden_csr(golden, "c1"), _P1(golden)
    x0 = np.random.RandomState(0).normal(0, 1, 1024)
    x, conv, err, it = ml.multigrid.amg_2_v(A, P, np.zeros(1024), x0, error_tol=1e-10)
    ref = golden["c1_amg2v_err_hist"]
    assert it == len(ref)
    # coarse solve: dense inverse vs SuperLU -> fp64 differences of ~1e-16 relative per cycle
    assert np.allclose(err, ref, rtol=1e-10, atol=1e-13 * ref[0])
    assert abs(conv - golden["c1_amg2v_err_conv"]) <= 1e-8
    x, conv, err, it = ml.multigrid.amg_2_v(A, P, np.zeros(1024), x0 / np.linalg.norm(x0),
                                            res_tol=1e-10)
    ref = golden["c1_amg2v_res_hist"]
    assert it == len(ref) and np.allclose(err, ref, rtol=1e-10, atol=1e-13 * ref[0])
    assert abs(conv - golden["c1_amg2v_res_conv"]) <= 1e-8


def test_amg_2_v_conv_quirks(golden, ml):
    A, P = golden_csr(golden, "c1"), _P1(golden)
    x0 = np.random.RandomState(0).normal(0, 1, 1024)
    got = [float(ml.multigrid.amg_2_v(A, P, np.zeros(1024), x0, error_tol=1e-300,
                                      max_iter=L)[1]) for L in range(1, 8)]
    assert np.allclose(got, golden["conv_quirk_values"], rtol=1e-10, atol=0)


def test_mlamg_two_level_history(golden, ml):
    A, P = golden_csr(golden, "c1"), _P1(golden)
    x0 = np.random.RandomState(0).normal(0, 1, 1024)
    for use_graph in (False, True):
        H = ml.hierarchy.Hierarchy.two_level(A, P)
        import torch
        xd = torch.as_tensor(x0).cuda()
        hist = H.cycle(torch.zeros(1024, dtype=torch.float64, device="cuda"), xd, 8,
                       use_graph=use_graph)
        ref = golden["c1_mlamg_hist"]
        assert len(hist) == 8
        assert np.allclose(hist, ref, rtol=1e-10, atol=1e-13 * ref[0])
        assert np.allclose(host(xd), golden["c1_mlamg_x8"], rtol=1e-9,
                           atol=1e-12 * np.abs(golden["c1_mlamg_x8"]).max())


def test_mlamg_tolerance_stop(golden, ml, oracle):
    A, P = golden_csr(golden, "c1"), _P1(golden)
    x0 = np.random.RandomState(0).normal(0, 1, 1024)
    xr, href = oracle.mlamg_amg_2_v(A, P, oracle.mlamg_dinv(A), np.zeros(1024), x0,
                                    max_iter=500, amg_rtol=1e-8)
    x, hist = ml.multigrid.amg_2_v_jacobi(A, P, np.zeros(1024), x0, tol=1e-8, history=True)
    assert len(hist) == len(href)
    assert np.allclose(hist, href, rtol=1e-8, atol=1e-14)


def test_amg_2_v_singular(golden_singular, ml):
    """Singular (Neumann) two-level solve, multigrid.py:178-187: device LSQR coarse solve + mean
    removal vs the reference's own histories (tests/golden/make_golden_singular.py).

    Tolerance: the reference's lsqr stops at atol = btol = 1e-6, so the cycle carries coarse
    solve errors of that size and its history depends on rounding. Measured on the CPU (scipy's
    own lsqr with math.fsum norms instead of BLAS ddot): the 2D case's history moves by 1.9e-7
    relative, its iterate by 4e-6 of its max, conv by 2e-9 — the bounds below are ~5x those. The
    1D case (res_tol, 60 cycles at conv ~0.78) is rounding-chaotic in the reference itself (the
    same experiment moves its history by up to 69 %): only its first cycles, its length and its
    convergence are compared."""
    from conftest import golden_csr
    g = golden_singular
    A, P = golden_csr(g, "n2d_A"), golden_csr(g, "n2d_P")
    x, conv, err, it = ml.multigrid.amg_2_v(A, P, g["n2d_b"], g["n2d_x0"], singular=True,
                                            max_iter=60, error_tol=1e-9)
    ref = g["n2d_err"]
    assert len(err) == len(ref) and it == len(ref)
    assert np.allclose(err, ref, rtol=1e-6, atol=0)
    assert abs(conv - float(g["n2d_conv"])) <= 1e-7
    assert np.abs(x - g["n2d_x"]).max() <= 2e-5 * np.abs(g["n2d_x"]).max()
    A, P = golden_csr(g, "n1d_A"), golden_csr(g, "n1d_P")
    x, conv, err, it = ml.multigrid.amg_2_v(A, P, g["n1d_b"], g["n1d_x0"], singular=True,
                                            max_iter=60, res_tol=1e-8)
    ref = g["n1d_err"]
    assert len(err) == len(ref)
    # fsum-norm scipy vs BLAS scipy: cycle 1 moves 1.6e-6, cycle 2 1.1e-4, cycle 6 1.5e-2
    assert abs(err[0] - ref[0]) <= 1e-5 * ref[0]
    assert err[-1] < 1e-3 * err[0] and 0.6 < conv < 0.95


def test_lsqr_matches_scipy(golden_singular, ml):
    """Device LSQR vs scipy.sparse.linalg.lsqr (the reference's coarse solver, multigrid.py:179)
    on the singular Galerkin operator and on a nonsymmetric rectangular least-squares problem:
    same stopping code and iteration count, solutions within fp64 rounding (norms are
    fixed-order device sums where scipy calls BLAS)."""
    import scipy.sparse.linalg as spla
    from conftest import golden_csr
    g = golden_singular
    A, P = golden_csr(g, "n2d_A"), golden_csr(g, "n2d_P")
    AH = (P.T @ A @ P).tocsr()
    rs = np.random.RandomState(3)
    M = sp.random(300, 120, density=0.05, random_state=rs, format="csr") + \
        sp.eye(300, 120, format="csr")
    for Mat, rhs in ((AH, P.T @ rs.randn(A.shape[0])), (M.tocsr(), rs.randn(300))):
        xr, istop, itn = spla.lsqr(Mat, rhs)[:3]
        x, istop_d, itn_d = ml.multigrid.lsqr(Mat, rhs)
        assert (istop_d, itn_d) == (istop, itn)
        # a different norm summation order inside scipy's own lsqr moves x by up to 1.1e-9 of
        # its max on these inputs (the inconsistent singular system is the sensitive one)
        assert np.abs(x - xr).max() <= 1e-8 * np.abs(xr).max()
    # zero right-hand side: x = 0, istop 0, no iteration (scipy's arnorm == 0 exit)
    x, istop_d, itn_d = ml.multigrid.lsqr(AH, np.zeros(AH.shape[0]))
    assert (istop_d, itn_d) == (0, 0) and not np.any(x)
