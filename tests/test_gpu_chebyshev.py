"""GPU: the polynomial (Chebyshev) smoother — the fused sweep in every storage format, the block
sweep, polynomial levels in both V-cycle executors, the Krylov solvers on them, and the pyamg
interface — against the host model of tests/poly_model.py (pyamg's relaxation.polynomial
restated; pyamg is absent, parity unpinned)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import poly_model
from conftest import golden_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.distributed
    import mlamg.hierarchy
    import mlamg.multigrid
    import mlamg.preconditioner
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def _bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _unsymmetric_257():
    """257 rows, random signs, an empty row (100) and a 70-entry row (200)."""
    rng = np.random.default_rng(12)
    M = sp.random(257, 257, density=5.0 / 257, random_state=rng, format="lil")
    M[100, :] = 0.0
    M[200, :] = 0.0
    M[200, rng.choice(257, 70, replace=False)] = 1.0
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    M.data[:] = rng.uniform(0.2, 1.0, M.nnz) * rng.choice([-1.0, 1.0], M.nnz)
    M.sort_indices()
    assert M.indptr[101] == M.indptr[100] and M.indptr[201] - M.indptr[200] == 70
    return M


MATRICES = ("p1d_1", "p1d_2", "p1d_65", "p2d_33x31", "c1", "unsym_257")


def _matrix(ml, golden, name):
    P = ml.problems
    if name.startswith("p1d_"):
        return sp.csr_matrix(P.poisson_1d(int(name[4:])))
    if name == "p2d_33x31":
        A = sp.csr_matrix(P.poisson_2d_5pt(33, 31))
        assert A.shape[0] == 1023
        return A
    if name == "c1":
        return golden_csr(golden, "c1")
    return _unsymmetric_257()


def _gershgorin(A):
    return float(abs(sp.csr_matrix(A)).sum(axis=1).max())


def _coeffs(ml, A, m):
    """m Chebyshev coefficients for rho = A's largest absolute row sum (bounded iterates)."""
    return ml.multigrid.chebyshev_coefficients(_gershgorin(A), degree=m)


# the formats whose row sums are scipy's, with the set_format argument of the autotune's list
SCIPY_FORMATS = (("csr_stream", 0), ("sell", 1), ("sorted", 0), ("long", 0), ("rowpat", 0),
                 ("sell_dict", 1))
REQUIRED_EVERYWHERE = ("csr_stream", "sell", "sorted", "long")
REQUIRED_ON_GRID = ("rowpat", "sell_dict")


def _set_format(Ad, fmt, arg):
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    try:
        Ad.set_format(fmt, arg)
        return True
    except MlamgError as e:
        if e.code != MLAMG_EUNSUPPORTED:
            raise
        return False


def _cases():
    for m in (1, 2, 3, 4):
        for iters in (1, 2):
            for zero in (False, True):
                for with_b in (True, False):
                    yield m, iters, zero, with_b


@pytest.mark.parametrize("name", MATRICES)
def test_sweep_bitwise_host_model(ml, torch_cuda, golden, name):
    """mlamg_poly_sweep equals the model bit for bit in every scipy-order format; with x_is_zero
    the iterate is filled with NaN first: it is not read."""
    torch = torch_cuda
    A = _matrix(ml, golden, name)
    n = A.shape[0]
    rng = np.random.default_rng(n)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    want = {}
    for m, iters, zero, with_b in _cases():
        want[m, iters, zero, with_b] = poly_model.sweep(A, x0, b if with_b else None,
                                                        _coeffs(ml, A, m), iters, zero)
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    bd = torch.as_tensor(b).cuda()
    taken = []
    for fmt, arg in SCIPY_FORMATS:
        if not _set_format(Ad, fmt, arg):
            assert fmt not in REQUIRED_EVERYWHERE, (name, fmt)
            assert not (name == "p2d_33x31" and fmt in REQUIRED_ON_GRID), (name, fmt)
            continue
        taken.append(fmt)
        for m in (1, 2, 3, 4):
            S = ml.multigrid.Polynomial(Ad, _coeffs(ml, A, m))
            for iters in (1, 2):
                for zero in (False, True):
                    for with_b in (True, False):
                        xd = (torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                              if zero else torch.as_tensor(x0).cuda())
                        S.sweep(xd, bd if with_b else None, iters, x_is_zero=zero)
                        assert _bits_equal(xd.cpu().numpy(), want[m, iters, zero, with_b]), \
                            (name, fmt, m, iters, zero, with_b)
    assert set(REQUIRED_EVERYWHERE) <= set(taken)


def _compose(ml, torch, Ad, c, x, b, iterations):
    """The sweep from the existing primitives on the same handle: mlamg_residual, then c * r and
    t + A h as separate torch operations."""
    from mlamg._lib import call, ptr, stream_ptr
    x = x.clone()
    for _ in range(iterations):
        r = torch.empty_like(x)
        call("mlamg_residual", Ad.handle, ptr(b), ptr(x), ptr(r), None, stream_ptr())
        h = float(c[0]) * r
        for ci in c[1:]:
            t = float(ci) * r
            h = t + Ad.matvec(h)
        x = x + h
    return x


@pytest.mark.parametrize("name", ["p2d_33x31", "unsym_257", "c1"])
def test_sweep_vector_format_is_the_composition(ml, torch_cuda, golden, name):
    """In the VECTOR format (canonical lane-parallel row sums, not scipy's) the sweep is bitwise
    the composition of the handle's own primitives; the same once in every other format."""
    torch = torch_cuda
    A = _matrix(ml, golden, name)
    n = A.shape[0]
    rng = np.random.default_rng(5)
    bd = torch.as_tensor(rng.standard_normal(n)).cuda()
    zb = torch.zeros_like(bd)
    x0 = torch.as_tensor(rng.standard_normal(n)).cuda()
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    for width in (64, 256):
        Ad.set_format("vector", width)
        for m, iters, zero, with_b in _cases():
            c = _coeffs(ml, A, m)
            S = ml.multigrid.Polynomial(Ad, c)
            xd = torch.full_like(x0, float("nan")) if zero else x0.clone()
            S.sweep(xd, bd if with_b else None, iters, x_is_zero=zero)
            ref = _compose(ml, torch, Ad, c, torch.zeros_like(x0) if zero else x0,
                           bd if with_b else zb, iters)
            assert torch.equal(xd.view(torch.int64), ref.view(torch.int64)), \
                (name, width, m, iters, zero, with_b)
    for fmt, arg in SCIPY_FORMATS:
        if not _set_format(Ad, fmt, arg):
            continue
        c = _coeffs(ml, A, 3)
        xd = x0.clone()
        ml.multigrid.Polynomial(Ad, c).sweep(xd, bd, 2)
        ref = _compose(ml, torch, Ad, c, x0, bd, 2)
        assert torch.equal(xd.view(torch.int64), ref.view(torch.int64)), (name, fmt)


@pytest.mark.parametrize("order", ["scipy", "canonical"])
@pytest.mark.parametrize("name", ["p2d_33x31", "unsym_257"])
def test_block_sweep_columns_bitwise_single(ml, torch_cuda, golden, name, order):
    """Column j of mlamg_poly_sweep_mv is bitwise mlamg_poly_sweep on column j: k = 1, 3, 8, 64,
    contiguous and padded blocks, in scipy order and (VECTOR format) in canonical order."""
    torch = torch_cuda
    A = _matrix(ml, golden, name)
    n = A.shape[0]
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    if order == "canonical":
        Ad.set_format("vector", 64)
    gen = torch.Generator(device="cpu").manual_seed(3)
    for m in (1, 2, 3, 4):
        S = ml.multigrid.Polynomial(Ad, _coeffs(ml, A, m))
        for k in (1, 3, 8, 64):
            for pad in (0, 3):
                Xw = torch.randn((n, k + pad), dtype=torch.float64, generator=gen).cuda()
                Bw = torch.randn((n, k + pad), dtype=torch.float64, generator=gen).cuda()
                for iters, zero, with_b in ((2, False, True), (1, True, True), (2, True, False),
                                            (1, False, False)):
                    X = Xw.clone()
                    Xb = X[:, :k]
                    if zero:
                        Xb.fill_(float("nan"))
                    S.sweep(Xb, Bw[:, :k] if with_b else None, iters, x_is_zero=zero)
                    if pad:  # the padding columns are untouched
                        assert torch.equal(X[:, k:], Xw[:, k:])
                    for j in sorted({0, k // 2, k - 1}):
                        xj = (torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                              if zero else Xw[:, j].clone())
                        S.sweep(xj, Bw[:, j].clone() if with_b else None, iters, x_is_zero=zero)
                        assert torch.equal(Xb[:, j].contiguous().view(torch.int64),
                                           xj.view(torch.int64)), (name, order, m, k, pad, j)


# ------------------------------------------------------------------------------- cycles
def _c1_P(golden):
    return sp.csr_matrix((golden["c1_P_data"], golden["c1_P_indices"], golden["c1_P_indptr"]),
                         shape=(1024, int(golden["c1_P_indices"].max()) + 1))


def _hierarchy(ml, golden, which):
    """(H, A, coarse matrix of the model, per-level coefficients). Every rho(A) is given as a
    number (the level operator's largest absolute row sum, an upper bound): no Arnoldi draws."""
    Hc = ml.hierarchy.Hierarchy
    if which in ("sa_2d", "sa_3d"):
        A = (sp.csr_matrix(ml.problems.poisson_2d_5pt(24)) if which == "sa_2d"
             else golden_csr(golden, "lap3d"))
        H0 = Hc.pyamg_sa(A, rho=[2.0] * 8)  # the level operators do not depend on the smoother
        rhos = [_gershgorin(L.A.to_scipy()) for L in H0.levels]
        H = Hc.pyamg_sa(A, rho=[2.0] * 8, smoother=("chebyshev", {"degree": 3}),
                        smoother_rho=rhos)
        assert [L.rho_A for L in H.levels] == rhos
        coarse = H.coarse_pinv
    elif which == "two_level_c1":
        A = golden_csr(golden, "c1")
        H = Hc.two_level(A, _c1_P(golden), smoother="chebyshev", degree=3,
                         smoother_rho=_gershgorin(A))
        coarse = np.linalg.pinv(H.Ac.to_scipy().toarray())
    else:  # "build": a weighted-Jacobi hierarchy given polynomial levels afterwards
        A = sp.csr_matrix(ml.problems.poisson_2d_5pt(48))
        H = Hc.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream",
                     coarse_format="exact")
        assert len(H.levels) >= 2
        H.set_polynomial_smoother([ml.multigrid.chebyshev_coefficients(
            _gershgorin(L.A.to_scipy()), 3) for L in H.levels])
        coarse = np.linalg.pinv(H.Ac.to_scipy().toarray())
    coeffs = [np.array(L.poly.coefficients, copy=True) for L in H.levels]
    return H, sp.csr_matrix(A), coarse, coeffs


def _close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("which", ["sa_2d", "sa_3d", "two_level_c1", "build"])
def test_cycles_with_polynomial_levels(ml, torch_cuda, golden, which):
    torch = torch_cuda
    from mlamg._lib import call
    H, A, coarse, coeffs = _hierarchy(ml, golden, which)
    assert all("polynomial (degree 3" in r["smoother"] for r in H.describe()[:-1])
    n = A.shape[0]
    rng = np.random.default_rng(9)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    bd, x0d = torch.as_tensor(b).cuda(), torch.as_tensor(x0).cuda()
    # captured graph == eager, three cycles (the second and third start from the kept residual)
    xe, xg = x0d.clone(), x0d.clone()
    he = H.cycle(bd, xe, 3, use_graph=False)
    hg = H.cycle(bd, xg, 3, use_graph=True)
    assert torch.equal(xe.view(torch.int64), xg.view(torch.int64)) and np.array_equal(he, hg)
    # zero right-hand side (b = NULL on the fine level) keeps the bits of a vector of zeros
    z1, z2 = x0d.clone(), x0d.clone()
    H.cycle(torch.zeros_like(bd), z1, 2)
    H.cycle_async(torch.zeros_like(bd), z2, 2, zero_rhs=False)
    assert torch.equal(z1.view(torch.int64), z2.view(torch.int64))
    # the model cycle
    levels = poly_model.model_levels(H)
    xm = poly_model.cycles(levels, coarse, b, x0, 3)
    print(f"{which}: max |device - model| / max|x| = "
          f"{np.abs(xe.cpu().numpy() - xm).max() / np.abs(xm).max():.3e}")
    _close(xe.cpu().numpy(), xm)
    # block cycle: column j bitwise the single cycle on column j
    k = 3
    B = torch.as_tensor(rng.standard_normal((n, k))).cuda()
    X = torch.as_tensor(rng.standard_normal((n, k))).cuda()
    Xs = X.clone()
    hm = H.cycle_multi(B, X, 2)
    for j in range(k):
        xj = Xs[:, j].clone()
        hj = H.cycle(B[:, j].clone(), xj, 2, use_graph=False)
        assert torch.equal(X[:, j].contiguous().view(torch.int64), xj.view(torch.int64)), j
        assert np.array_equal(hm[:, j], hj)
    # other cycle shapes, and two iterations per sweep
    for nu_pre, nu_post, iters in ((2, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 2)):
        H.set_polynomial_smoother(coeffs, iters)
        call("mlamg_hier_set_smoothing", H.handle, nu_pre, nu_post)
        xd = x0d.clone()
        H.cycle(bd, xd, 2)
        xm = poly_model.cycles(poly_model.model_levels(H, iters), coarse, b, x0, 2, nu_pre,
                               nu_post)
        print(f"{which} V({nu_pre},{nu_post}) x{iters}: "
              f"{np.abs(xd.cpu().numpy() - xm).max() / np.abs(xm).max():.3e}")
        _close(xd.cpu().numpy(), xm)
        Xm = Xs.clone()
        H.cycle_multi(B, Xm, 1, history=False)
        x1 = Xs[:, 1].clone()
        H.cycle(B[:, 1].clone(), x1, 1, history=False)
        assert torch.equal(Xm[:, 1].contiguous().view(torch.int64), x1.view(torch.int64))
    call("mlamg_hier_set_smoothing", H.handle, 1, 1)


@pytest.mark.parametrize("which", ["build", "pyamg_gs", "two_level_gs"])
def test_removing_the_polynomial_restores_the_recipe(ml, torch_cuda, golden, which):
    """set_polynomial_smoother(None): the cycle is bitwise what it was (Jacobi fusions, the
    Gauss-Seidel handles), in a V(1,1) and a V(2,1)."""
    torch = torch_cuda
    from mlamg._lib import call
    Hc = ml.hierarchy.Hierarchy
    if which == "build":
        A = sp.csr_matrix(ml.problems.poisson_2d_5pt(48))
        H = Hc.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream", coarse_format="exact")
    elif which == "pyamg_gs":
        A = sp.csr_matrix(ml.problems.poisson_2d_5pt(24))
        H = Hc.pyamg_sa(A, rho=[2.0] * 8)
    else:
        A = golden_csr(golden, "c1")
        H = Hc.two_level(A, _c1_P(golden), smoother="gauss_seidel")
    n = A.shape[0]
    rng = np.random.default_rng(1)
    bd = torch.as_tensor(rng.standard_normal(n)).cuda()
    x0 = torch.as_tensor(rng.standard_normal(n)).cuda()
    before_desc = H.describe()

    def run():
        out = []
        for nu in ((1, 1), (2, 1)):
            call("mlamg_hier_set_smoothing", H.handle, *nu)
            x = x0.clone()
            out.append((H.cycle(bd, x, 3), x))
        call("mlamg_hier_set_smoothing", H.handle, 1, 1)
        return out

    before = run()
    H.set_polynomial_smoother(ml.multigrid.chebyshev_coefficients(_gershgorin(A), 3))
    assert "polynomial" in H.describe()[0]["smoother"]
    with_poly = run()
    assert not torch.equal(with_poly[0][1], before[0][1])
    H.set_polynomial_smoother(None)
    assert H.describe() == before_desc
    for (h0, xa), (h1, xb) in zip(before, run()):
        assert np.array_equal(h0, h1) and torch.equal(xa.view(torch.int64), xb.view(torch.int64))


# ------------------------------------------------------------------------------- solvers
def test_krylov_solvers_on_a_chebyshev_hierarchy(ml, torch_cuda, golden):
    torch = torch_cuda
    H, A, _, _ = _hierarchy(ml, golden, "sa_2d")
    n = A.shape[0]
    rng = np.random.default_rng(21)
    B = rng.standard_normal((n, 3))
    nb = np.linalg.norm(B, axis=0)
    cols = []
    for j in range(3):
        x, info = H.gmres(B[:, j].copy(), rtol=1e-8, restart=30, return_info=True)
        assert info["info"] == 0
        assert np.linalg.norm(B[:, j] - A @ x) <= 1e-8 * nb[j]
        cols.append((x, info))
    X, infos = H.gmres_multi(torch.as_tensor(B).cuda(), rtol=1e-8, restart=30, return_info=True)
    Xh = X.cpu().numpy()
    for j, (x, info) in enumerate(cols):
        assert infos["info"][j] == 0 and infos["inner_iters"][j] == info["inner_iters"]
        assert _bits_equal(Xh[:, j], x), j
    xh, ih = H.gmres_householder(B[:, 0].copy(), tol=1e-8, maxiter=100, return_info=True)
    # pyamg's stop test is on the preconditioned residual
    assert ih["info"] == 0 and ih["residuals"][-1] <= 1e-8 * ih["residuals"][0]
    assert np.linalg.norm(B[:, 0] - A @ xh) <= 1e-6 * nb[0]


def test_polynomial_levels_with_a_pcg_coarse_solve(ml, torch_cuda):
    """Hierarchy.build on a 48^2 grid with the dense limit lowered so the coarsest solve is PCG
    (host driven: the cycle runs eagerly whatever use_graph says): cycles without error, the
    same bits either way, the block cycle's column too."""
    torch = torch_cuda
    A = sp.csr_matrix(ml.problems.poisson_2d_5pt(48))
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_levels=2, finalize=False)
    H.apply_formats("csr_stream", "exact")
    H._finalize(1, 1, dense_max=100)
    assert H.pcg is not None
    H.set_polynomial_smoother(ml.multigrid.chebyshev_coefficients(_gershgorin(A), 3))
    b = torch.as_tensor(np.random.default_rng(2).standard_normal(A.shape[0])).cuda()
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    h1 = H.cycle(b, x1, 4, use_graph=True)
    h2 = H.cycle(b, x2, 4, use_graph=False)
    assert torch.equal(x1.view(torch.int64), x2.view(torch.int64)) and np.array_equal(h1, h2)
    assert len(h1) == 4 and (np.diff(h1) < 0).all()
    X = torch.zeros((A.shape[0], 2), dtype=torch.float64, device="cuda")
    Bm = torch.stack([b, 2.0 * b], dim=1).contiguous()
    H.cycle_multi(Bm, X, 4, history=False)
    assert torch.equal(X[:, 0].contiguous().view(torch.int64), x1.view(torch.int64))


# ------------------------------------------------------------------------------- interface
def test_pyamg_compat_polynomial_equals_model(ml, torch_cuda, golden):
    from mlamg.pyamg_compat.relaxation import chebyshev, relaxation
    A = _matrix(ml, golden, "p2d_33x31")
    rng = np.random.default_rng(6)
    b = rng.standard_normal(A.shape[0])
    for degree in (1, 3):
        c = -chebyshev.chebyshev_polynomial_coefficients(8.0 / 30, 8.8, degree)[:-1]
        x = rng.standard_normal(A.shape[0])
        want = poly_model.sweep(A, x, b, c, 2)
        relaxation.polynomial(A, x, b, c, iterations=2)
        assert _bits_equal(x, want)


def test_smoothed_aggregation_solver_takes_chebyshev(ml, torch_cuda):
    from mlamg.pyamg_compat import aggregation
    A = sp.csr_matrix(ml.problems.poisson_2d_5pt(40))
    np.random.seed(0)  # approximate_spectral_radius draws from numpy's global generator
    s = aggregation.smoothed_aggregation_solver(A, presmoother="chebyshev",
                                                postsmoother="chebyshev")
    assert all(L.poly is not None and L.poly.coefficients.size == 3 for L in s.H.levels)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    x, info = s.solve(b, tol=1e-8, maxiter=100, return_info=True)
    assert info == 0 and np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)
    s4 = aggregation.smoothed_aggregation_solver(
        A, presmoother=("chebyshev", {"degree": 4, "iterations": 2}),
        postsmoother=("chebyshev", {"degree": 4, "iterations": 2}))
    assert s4.H.levels[0].poly.coefficients.size == 4 and s4.H.poly_iterations == 2
    with pytest.raises(NotImplementedError):
        aggregation.smoothed_aggregation_solver(A, presmoother="chebyshev")
    with pytest.raises(NotImplementedError):
        aggregation.smoothed_aggregation_solver(
            A, presmoother=("chebyshev", {"degree": 3}), postsmoother=("chebyshev", {"degree": 2}))


def test_multilevel_pc_chebyshev_option(ml, torch_cuda):
    A = ml.problems.poisson_2d_5pt(48)

    class PC:
        def getOperators(self):
            return None, A

        def getOptionsPrefix(self):
            return ""

    store = ml.preconditioner._Options.store
    store["pyamg_amg_smoother"] = "chebyshev"
    store["pyamg_amg_chebyshev_degree"] = 4
    try:
        np.random.seed(1)
        pc = ml.preconditioner.MultilevelPC()
        pc.initialize(PC())
        assert pc.H.recipe == "pyamg_sa"
        assert all(L.poly is not None and L.poly.coefficients.size == 4 for L in pc.H.levels)
        b = np.random.default_rng(0).standard_normal(A.shape[0])
        y = np.zeros_like(b)
        pc.apply(PC(), b, y)
        assert np.linalg.norm(b - A @ y) <= 1e-7 * np.linalg.norm(b)
        store["pyamg_amg_smoother"] = "sor"
        with pytest.raises(ValueError):
            ml.preconditioner.MultilevelPC().initialize(PC())
    finally:
        store.pop("pyamg_amg_smoother", None)
        store.pop("pyamg_amg_chebyshev_degree", None)


def test_invalid_arguments_are_refused_before_any_launch(ml, torch_cuda, golden):
    torch = torch_cuda
    from mlamg._lib import MLAMG_EINVAL, MlamgError, call
    A = _matrix(ml, golden, "p1d_65")
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    for bad in ([1.0, float("nan")], [float("inf")], []):
        with pytest.raises(MlamgError) as e:
            ml.multigrid.Polynomial(Ad, bad)
        assert e.value.code == MLAMG_EINVAL
    R = ml.sparse.DeviceCSR.from_scipy(sp.csr_matrix(np.ones((3, 5))))
    with pytest.raises(MlamgError) as e:
        ml.multigrid.Polynomial(R, [1.0])
    assert e.value.code == MLAMG_EINVAL
    S = ml.multigrid.Polynomial(Ad, [0.1, 0.2])
    rows, m = ctypes.c_int64(), ctypes.c_int()
    call("mlamg_poly_info", S.handle, ctypes.byref(rows), ctypes.byref(m))
    assert (rows.value, m.value) == (65, 2)
    x = torch.zeros(65, dtype=torch.float64, device="cuda")
    with pytest.raises(MlamgError) as e:
        S.sweep(x, x)  # b == x
    assert e.value.code == MLAMG_EINVAL
    with pytest.raises(MlamgError) as e:
        S.sweep(x, None, iterations=-1)
    assert e.value.code == MLAMG_EINVAL
    # a handle of another size on a hierarchy level
    H = ml.hierarchy.Hierarchy.pyamg_sa(sp.csr_matrix(ml.problems.poisson_2d_5pt(24)),
                                        rho=[2.0] * 8)
    with pytest.raises(MlamgError) as e:
        call("mlamg_hier_set_level_polynomial", H.handle, 0, S.handle, 1)
    assert e.value.code == MLAMG_EINVAL
    with pytest.raises(ValueError):
        H.set_polynomial_smoother([[0.1], [0.2]] * 4)  # not one set per level
    with pytest.raises(NotImplementedError):
        ml.hierarchy.Hierarchy.pyamg_sa(A, smoother="sor")


def test_distributed_hierarchy_refuses_polynomial_levels(ml, torch_cuda):
    A = sp.csr_matrix(ml.problems.poisson_2d_5pt(48))
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream",
                                     coarse_format="exact")
    H.set_polynomial_smoother(ml.multigrid.chebyshev_coefficients(8.0, 3))
    with pytest.raises(NotImplementedError, match="polynomial"):
        ml.distributed.DistributedHierarchy(H, comm=None)
