"""GPU: the multi-vector (n x k) path — SpMM and its epilogues, per-column norms and mean removal,
the dense coarse solve on a block, the block V-cycle, amg_loss (ns/model/loss.py:32-96).

The acceptance criterion needs no new oracle: column j of every multi-vector result is bitwise
the existing single-vector result on column j (scipy's csr_matvecs sums every column of A @ X
exactly as csr_matvec sums A @ x). All comparisons are np.array_equal unless stated."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 3, 8, 16, 17, 50, 64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.hierarchy
    import mlamg.loss
    import mlamg.multigrid
    import mlamg.preconditioner
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


def _matrix(ml, name):
    if name == "poisson_33x31":  # 1,023 rows: the last row block is not full
        return ml.problems.poisson_2d_5pt(33, 31).tocsr()
    if name == "lap3d_grid":  # the reference's demos/laplace_3d.grid: 1,331 rows, 15-point
        g = np.load(os.path.join(HERE, "golden", "laplace_3d_grid.npz"))
        return sp.csr_matrix((g["data"], g["indices"], g["indptr"]))
    if name == "rect_700x300":  # rectangular, empty first and last rows
        A = sp.random(700, 300, density=0.02, random_state=np.random.RandomState(5),
                      format="lil")
        A[0, :] = 0
        A[699, :] = 0
        A = A.tocsr()
        A.eliminate_zeros()
        return A
    if name == "long_row_40x6000":  # row 7 has 6,000 entries: over the 2,048-nonzero block
        rs = np.random.RandomState(6)
        A = sp.lil_matrix((40, 6000))
        for i in range(40):
            m = rs.randint(0, 6)
            cols = rs.choice(6000, size=m, replace=False)
            A[i, cols] = rs.standard_normal(m)
        A[7, :] = rs.standard_normal(6000)
        return A.tocsr()
    if name == "one_by_one":
        return sp.csr_matrix(np.array([[2.5]]))
    raise KeyError(name)


MATRICES = ("poisson_33x31", "lap3d_grid", "rect_700x300", "long_row_40x6000", "one_by_one")


@pytest.mark.parametrize("name", MATRICES)
def test_spmm_matches_matvec_and_scipy(ml, torch_cuda, name):
    """A.matmat(X)[:, j] is bitwise A.matvec(X[:, j]) and scipy's A @ X, for every k and with
    each exact format active on the handle (the SpMM reads the CSR arrays only)."""
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    A = _matrix(ml, name)
    if name == "long_row_40x6000":
        assert np.diff(A.indptr)[7] == 6000
    if name == "rect_700x300":
        assert A.indptr[1] == 0 and A.indptr[-1] == A.indptr[-2]
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    ran = []
    for fmt in ("csr_stream", "sell", "sorted", "long"):
        try:
            Ad.set_format(fmt)
        except MlamgError as e:  # a format that does not accept this matrix
            assert e.code == MLAMG_EUNSUPPORTED and fmt != "csr_stream", (fmt, str(e))
            continue
        ran.append(fmt)
        for k in KS:
            Xh = np.random.RandomState(1).standard_normal((A.shape[1], k))
            X = dev(torch, Xh)
            Y = host(Ad.matmat(X))
            ref = A @ Xh
            assert Y.shape == ref.shape
            assert np.array_equal(Y, ref), (fmt, k)
            Y2 = host(Ad @ X)
            assert np.array_equal(Y2, Y)
            for j in range(k):
                yj = host(Ad.matvec(X[:, j].contiguous()))
                assert np.array_equal(Y[:, j], yj), (fmt, k, j)
    assert "csr_stream" in ran


@pytest.mark.parametrize("k", (3, 8))
def test_spmm_strides(ml, torch_cuda, k):
    """X and out as column slices of wider buffers (k = 3 in a 4-wide, k = 8 in a 9-wide
    buffer: an odd leading dimension, rows not 16-byte aligned): the contiguous result, and
    the columns outside the slice untouched."""
    torch = torch_cuda
    A = _matrix(ml, "poisson_33x31")
    n = A.shape[0]
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    Xh = np.random.RandomState(1).standard_normal((n, k))
    want = host(Ad.matmat(dev(torch, Xh)))
    buf = torch.full((n, k + 1), 7.25, dtype=torch.float64, device="cuda")
    buf[:, :k] = dev(torch, Xh)
    X = buf[:, :k]
    assert X.stride(0) == k + 1 and X.data_ptr() == buf.data_ptr()
    sentinel = -123.5
    for width, off in ((k + 1, 0), (k + 1, 1), (k + 2, 1)):
        obuf = torch.full((n, width), sentinel, dtype=torch.float64, device="cuda")
        out = obuf[:, off:off + k]
        res = Ad.matmat(X, out=out)
        assert res.data_ptr() == out.data_ptr()
        o = host(obuf)
        assert np.array_equal(o[:, off:off + k], want), (width, off)
        rest = np.delete(o, np.s_[off:off + k], axis=1)
        assert np.all(rest == sentinel), (width, off)
    assert np.all(host(buf)[:, k] == 7.25)
    with pytest.raises(ValueError):
        Ad.matmat(buf[:, ::2])  # column stride 2
    with pytest.raises(TypeError):
        Ad.matmat(X.float())
    with pytest.raises(TypeError):
        Ad.matmat(X.cpu())


def _call(name, *args):
    from mlamg._lib import call
    return call(name, *args)


def test_alpha_beta_and_epilogues(ml, torch_cuda):
    """alpha/beta, residual (with B and B = NULL) and its norms, Jacobi sweeps of both
    ping-pong parities: per column the single-vector entry points' bits."""
    torch = torch_cuda
    from mlamg._lib import ptr, stream_ptr
    A = _matrix(ml, "poisson_33x31")
    n = A.shape[0]
    k = 6
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    rs = np.random.RandomState(2)
    X = dev(torch, rs.standard_normal((n, k)))
    B = dev(torch, rs.standard_normal((n, k)))
    Y0 = dev(torch, rs.standard_normal((n, k)))
    s = stream_ptr()
    # alpha = -0.5, beta = 2
    Y = Y0.clone()
    Ad.matmat(X, out=Y, alpha=-0.5, beta=2.0)
    for j in range(k):
        yj = Y0[:, j].contiguous()
        Ad.matvec(X[:, j].contiguous(), out=yj, alpha=-0.5, beta=2.0)
        assert np.array_equal(host(Y[:, j]), host(yj)), j
    # beta = 0 with alpha != 1
    Y = Ad.matmat(X, alpha=3.0)
    for j in range(k):
        yj = Ad.matvec(X[:, j].contiguous(), alpha=3.0)
        assert np.array_equal(host(Y[:, j]), host(yj)), j
    # residual and its norms
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    for Bm in (B, None):
        R = torch.empty((n, k), dtype=torch.float64, device="cuda")
        norms = torch.empty(k, dtype=torch.float64, device="cuda")
        _call("mlamg_residual_mv", Ad.handle, ptr(Bm), k, ptr(X), k, ptr(R), k, k, ptr(norms), s)
        for j in range(k):
            r = torch.empty(n, dtype=torch.float64, device="cuda")
            bj = B[:, j].contiguous() if Bm is not None else zero
            _call("mlamg_residual", Ad.handle, ptr(bj), ptr(X[:, j].contiguous()), ptr(r), None, s)
            assert np.array_equal(host(R[:, j]), host(r)), j
            nj = torch.empty(1, dtype=torch.float64, device="cuda")
            _call("mlamg_norm2", ptr(R[:, j].contiguous()), n, ptr(nj), s)
            assert host(norms)[j] == host(nj)[0], j
    # Jacobi
    dinv = Ad.diag_inv(2.0 / 3.0)
    for nu in (1, 2, 3):
        Xm = X.clone()
        T = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
        _call("mlamg_jacobi_mv", Ad.handle, ptr(dinv), ptr(B), k, ptr(Xm), k, ptr(T), k, k, nu, s)
        for j in range(k):
            xj = X[:, j].contiguous()
            tj = torch.empty_like(xj)
            _call("mlamg_jacobi", Ad.handle, ptr(dinv), ptr(B[:, j].contiguous()), ptr(xj),
                  ptr(tj), nu, s)
            assert np.array_equal(host(Xm[:, j]), host(xj)), (nu, j)


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


def test_restrict_and_prolong_add(ml, torch_cuda):
    torch = torch_cuda
    from mlamg._lib import ptr, stream_ptr
    m = 32
    A = ml.problems.poisson_2d_5pt(m).tocsr()
    P = _sa_P(A, _agg_matrix(ml, m))
    H = ml.hierarchy.Hierarchy.two_level(A, P)
    L = H.levels[0]
    n, nc = L.P.shape
    k = 6
    rs = np.random.RandomState(3)
    Rf = dev(torch, rs.standard_normal((n, k)))
    E = dev(torch, rs.standard_normal((nc, k)))
    X0 = dev(torch, rs.standard_normal((n, k)))
    s = stream_ptr()
    Bc = torch.empty((nc, k), dtype=torch.float64, device="cuda")
    _call("mlamg_restrict_mv", L.R.handle, ptr(Rf), k, ptr(Bc), k, k, s)
    X = X0.clone()
    _call("mlamg_prolong_add_mv", L.P.handle, ptr(E), k, ptr(X), k, k, s)
    for j in range(k):
        bc = torch.empty(nc, dtype=torch.float64, device="cuda")
        _call("mlamg_restrict", L.R.handle, ptr(Rf[:, j].contiguous()), ptr(bc), s)
        assert np.array_equal(host(Bc[:, j]), host(bc)), j
        xj = X0[:, j].contiguous()
        _call("mlamg_prolong_add", L.P.handle, ptr(E[:, j].contiguous()), ptr(xj), s)
        assert np.array_equal(host(X[:, j]), host(xj)), j


@pytest.mark.parametrize("n", (1, 255, 256, 257, 300001))
def test_norm2_and_remove_mean(ml, torch_cuda, n):
    """Per-column norms and mean removal against the single forms; n = 300,001 exceeds
    1024 x 256 (and 512 x 256), so both grid-stride loops wrap."""
    torch = torch_cuda
    from mlamg._lib import ptr, stream_ptr
    k = 5
    s = stream_ptr()
    buf = dev(torch, np.random.RandomState(n).standard_normal((n, k + 2)) + 0.25)
    for X in (buf[:, :k].contiguous(), buf[:, 1:1 + k]):
        ld = X.stride(0) if n > 1 else max(X.stride(0), k)
        out = torch.empty(k, dtype=torch.float64, device="cuda")
        _call("mlamg_norm2_mv", ptr(X), ld, n, k, ptr(out), s)
        cols = [X[:, j].contiguous() for j in range(k)]
        for j in range(k):
            nj = torch.empty(1, dtype=torch.float64, device="cuda")
            _call("mlamg_norm2", ptr(cols[j]), n, ptr(nj), s)
            assert host(out)[j] == host(nj)[0], (n, j)
        before = host(buf).copy()
        _call("mlamg_remove_mean_mv", ptr(X), ld, n, k, s)
        for j in range(k):
            _call("mlamg_remove_mean", ptr(cols[j]), n, s)
            assert np.array_equal(host(X[:, j]), host(cols[j])), (n, j)
        if X.data_ptr() != buf.data_ptr() and X.stride(0) == k + 2:  # the slice: neighbours kept
            after = host(buf)
            assert np.array_equal(after[:, 0], before[:, 0])
            assert np.array_equal(after[:, k + 1], before[:, k + 1])


def _upwind(ml, m, c=0.5):
    """2D 5-point Laplacian plus first-order upwind convection (tests/test_gpu_coarse_pcg.py): its
    Galerkin coarse operator is not symmetric."""
    A = ml.problems.poisson_2d_5pt(m).tocsr()
    n = A.shape[0]
    return sp.csr_matrix(A + c * (sp.eye(n) - sp.eye(n, k=-1)))


@pytest.mark.parametrize("method", (1, 0, 2))
def test_dense_solve_mv(ml, torch_cuda, method):
    torch = torch_cuda
    from mlamg._lib import ptr, stream_ptr
    if method == 1:  # SPD Galerkin operator, 100 rows
        A = ml.problems.poisson_2d_5pt(30).tocsr()
        P = _sa_P(A, _agg_matrix(ml, 30))
        M = sp.csr_matrix(P.T @ A @ P)
        assert M.shape[0] == 100
    elif method == 0:  # upwind convection-diffusion coarse operator: not symmetric
        A = _upwind(ml, 48)
        P = _sa_P(ml.problems.poisson_2d_5pt(48).tocsr(), _agg_matrix(ml, 48))
        M = sp.csr_matrix(P.T @ A @ P)
    else:  # SPD, >= 2,048 rows: the factor kept, two triangular passes
        M = ml.problems.poisson_2d_5pt(46).tocsr()
        assert M.shape[0] >= 2048
    n = M.shape[0]
    k = 7
    Md = ml.sparse.DeviceCSR.from_scipy(M)
    h = ctypes.c_void_p()
    _call("mlamg_dense_create", Md.handle, ctypes.byref(h), stream_ptr())
    try:
        meth = ctypes.c_int()
        _call("mlamg_dense_info", h, ctypes.byref(meth), None)
        assert meth.value == method
        wide = dev(torch, np.random.RandomState(4).standard_normal((n, k + 1)))
        for B in (wide[:, :k].contiguous(), wide[:, :k]):
            X = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
            _call("mlamg_dense_solve_mv", h, ptr(B), B.stride(0), ptr(X), k, k, stream_ptr())
            for j in range(k):
                x = torch.empty(n, dtype=torch.float64, device="cuda")
                _call("mlamg_dense_solve", h, ptr(B[:, j].contiguous()), ptr(x), stream_ptr())
                assert np.array_equal(host(X[:, j]), host(x)), j
        ref = np.linalg.solve(M.toarray(), host(wide[:, :k]))
        assert np.allclose(host(X), ref, rtol=1e-9, atol=1e-11 * np.abs(ref).max())
    finally:
        _call("mlamg_dense_destroy", h)


def _single_loop(torch, H, b, x, n_cycles, norm, remove_mean):
    """n_cycles single-vector cycles on (b, x), each followed by the mean removal (if asked)
    and mlamg_norm2 of the freshly computed residual (or of x): the history cycle_multi is
    defined by."""
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
def hierarchies(ml, torch_cuda):
    Hs = {}
    A = ml.problems.poisson_2d_5pt(48)
    Hs["multilevel"] = ml.hierarchy.Hierarchy.build(A, max_coarse=100, fine_format="csr_stream",
                                                    coarse_format="exact")
    assert Hs["multilevel"].n_levels >= 3
    A2 = ml.problems.poisson_2d_5pt(32).tocsr()
    Hs["two_level"] = ml.hierarchy.Hierarchy.two_level(A2, _sa_P(A2, _agg_matrix(ml, 32)))
    return Hs


@pytest.mark.parametrize("nu", ((1, 1), (2, 1), (0, 1), (1, 0), (2, 2), (0, 0)))
@pytest.mark.parametrize("which", ("multilevel", "two_level"))
def test_block_cycle_matches_single_cycles(ml, torch_cuda, hierarchies, which, nu):
    torch = torch_cuda
    H = hierarchies[which]
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
            if Bm is None:  # B = None equals an all-zero B
                X3 = X0.clone()
                hist3 = H.cycle_multi(torch.zeros_like(B), X3, cycles, norm=norm,
                                      remove_mean=remove_mean)
                assert np.array_equal(host(X), host(X3)) and np.array_equal(hist, hist3)
        # a column slice of a wider iterate, history off
        wide = torch.full((n, k + 1), 3.0, dtype=torch.float64, device="cuda")
        wide[:, :k] = X0
        assert H.cycle_multi(B, wide[:, :k], cycles, history=False) is None
        Xc = X0.clone()
        H.cycle_multi(B, Xc, cycles, history=False)
        assert np.array_equal(host(wide)[:, :k], host(Xc)) and np.all(host(wide)[:, k] == 3.0)
    finally:
        _call("mlamg_hier_set_smoothing", H.handle, 1, 1)


def test_refusals(ml, torch_cuda):
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    A = ml.problems.poisson_2d_5pt(32).tocsr()
    n = A.shape[0]
    P = _sa_P(A, _agg_matrix(ml, 32))
    X = torch.ones((n, 4), dtype=torch.float64, device="cuda")
    H = ml.hierarchy.Hierarchy.two_level(A, P, smoother="gauss_seidel")
    with pytest.raises(MlamgError, match="Gauss-Seidel") as ei:
        H.cycle_multi(None, X, 1)
    assert ei.value.code == MLAMG_EUNSUPPORTED
    Hv = ml.hierarchy.Hierarchy.build(ml.problems.poisson_2d_5pt(48), max_coarse=100,
                                      coarse_format="vector")
    fmts = [M.get_format()[0] for L in Hv.levels for M in (L.A, L.P, L.R)]
    if "vector" not in fmts:  # rows too short for the family rule: put one operator there
        Hv.levels[1].A.set_format("vector", 64)
    Xv = torch.ones((48 * 48, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(MlamgError, match="VECTOR") as ei:
        Hv.cycle_multi(None, Xv, 1)
    assert ei.value.code == MLAMG_EUNSUPPORTED
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    with pytest.raises(ValueError):
        Ad @ torch.ones((n, 65), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        H.cycle_multi(None, torch.ones((n, 65), dtype=torch.float64, device="cuda"), 1)


def _amg_loss_restated(A, P, k, tot_num_loop=5, no_prerelax=1, no_postrelax=1):
    """ns/model/loss.py:48-96 restated in fp64 numpy/scipy (the reference holds x in fp32 and
    solves the coarse system in fp64 with torch_sparse_solve; here SuperLU throughout)."""
    omega = 2.0 / 3.0
    Dinv = sp.diags((1.0 / A.diagonal()) * omega)
    Pt = sp.csr_matrix(P.T)
    lu = spla.splu(sp.csc_matrix(Pt @ A @ P))
    n = A.shape[0]
    np.random.seed(0)
    x = np.random.normal(0, 1, (n, k))
    x = x / np.linalg.norm(x, 2, axis=0)
    errs = np.zeros((tot_num_loop + 1, k))
    for it in range(tot_num_loop + 1):
        for _ in range(no_prerelax):
            x = x - Dinv @ (A @ x)
        r_H = Pt @ (A @ x)
        e_H = lu.solve(-r_H)
        x = x + P @ e_H
        for _ in range(no_postrelax):
            x = x - Dinv @ (A @ x)
        x = x - x.mean(0)
        errs[it] = np.linalg.norm(x, 2, axis=0)
    convs = (errs[-1] / errs[-3]) ** (1 / 2)
    e = np.exp(convs)
    return (e / e.sum()) @ convs, convs, errs


def test_amg_loss(ml, torch_cuda):
    """amg_loss on poisson_2d_5pt(24) with a box-aggregate SA prolongator and 8 test vectors:
    its history is bitwise the single-vector loop (norm of x, mean removed), and agrees with the
    fp64 restatement of loss.py within the project's SuperLU-versus-dense bounds (history rtol
    1e-10, factors 1e-8: SURVEY §8(d), tests/test_gpu_coarse_pcg.py)."""
    torch = torch_cuda
    m, k = 24, 8
    A = ml.problems.poisson_2d_5pt(m).tocsr()
    P = _sa_P(A, _agg_matrix(ml, m))
    loss, convs, errs = ml.loss.amg_loss(P, A, k, return_factors=True)
    assert errs.shape == (6, k) and convs.shape == (k,)
    assert ml.loss.amg_loss(P, A, k) == loss
    # bit for bit: the single-vector loop on the same starting vectors
    np.random.seed(0)
    x0 = np.random.normal(0, 1, (A.shape[0], k))
    x0 = x0 / np.linalg.norm(x0, 2, axis=0)
    H = ml.hierarchy.Hierarchy.two_level(A, P, omega=2.0 / 3.0, nu_pre=1, nu_post=1)
    for j in range(k):
        hj = _single_loop(torch, H, None, dev(torch, x0[:, j]), 6, "x", True)
        assert np.array_equal(errs[:, j], hj), (j, errs[:, j], hj)
    # other operator types and given vectors: the same bits
    l2, c2, e2 = ml.loss.amg_loss(ml.sparse.DeviceCSR.from_scipy(P), ml.sparse.DeviceCSR.from_scipy(A),
                                  dev(torch, x0), return_factors=True)
    assert l2 == loss and np.array_equal(e2, errs)
    # the restatement
    rl, rc, re = _amg_loss_restated(A, P, k)
    print("amg_loss errs max rel diff", np.abs(errs / re - 1).max(),
          "convs max abs diff", np.abs(convs - rc).max(), "loss", loss, rl)
    assert np.allclose(errs, re, rtol=1e-10, atol=0), (errs, re)
    assert np.abs(convs - rc).max() <= 1e-8
    assert abs(loss - rl) <= 1e-8


def test_precondition_block(ml, torch_cuda, hierarchies):
    torch = torch_cuda
    H = hierarchies["multilevel"]
    n = H.levels[0].A.shape[0]
    k = 5
    Bh = np.random.RandomState(9).standard_normal((n, k))
    B = dev(torch, Bh)
    Z = H.precondition(B)
    assert isinstance(Z, torch.Tensor) and tuple(Z.shape) == (n, k)
    Zh = ml.preconditioner.precondition(H, Bh)
    assert isinstance(Zh, np.ndarray) and np.array_equal(Zh, host(Z))
    for j in range(k):
        zj = H.precondition(B[:, j].contiguous())
        assert np.array_equal(host(Z[:, j]), host(zj)), j
