"""GPU: the gradient of amg_loss with respect to the prolongator's stored values
(mlamg.loss.amg_loss_and_grad, amg_loss_values).

The independent reference is `reference_loss_and_grad` below: ns/model/loss.py:48-96 restated
densely in torch fp64 on the CPU, with P built from its values by index_put,
torch.linalg.solve for the coarse system and .backward(). Nothing of the library runs in it.

Measured on the MI355X (printed by test_gradient_matches_autograd),
max |grad - ref| / max |ref|: 2.4e-15 (Poisson 12^2), 3.2e-15 (non-symmetric 12^2), 1.9e-15
(Poisson 16^2, nu = (2, 2)), 6.3e-15 (Poisson 24^2), 2.5e-15 (non-symmetric 9^2); the numpy
adjoint on the CPU gave 6.5e-16 .. 1.5e-15. The assertion is 100 times the worst case and never
above 1e-9, the cap the feature was specified with. The central differences agreed with
grad . d to 3.2e-11 .. 2.0e-8 relative (bound 1e-6)."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

# worst max|grad - ref| / max|ref| over the five problems, measured on the device
WORST_MEASURED = 6.3e-15
GRAD_RTOL = min(100.0 * WORST_MEASURED, 1e-9)
FD_H = 1e-5
FD_RTOL = 1e-6

#            name                grid box  k  nu      non-symmetric
PROBLEMS = (("poisson12_box3", 12, 3, 4, (1, 1), False),
            ("nonsym12_box3", 12, 3, 4, (1, 1), True),
            ("poisson16_box4_nu22", 16, 4, 8, (2, 2), False),
            ("poisson24_box3", 24, 3, 8, (1, 1), False),
            ("nonsym9_box2_nu01", 9, 2, 3, (0, 1), True))
NAMES = tuple(p[0] for p in PROBLEMS)
TOT = 5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.loss
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def _problem(ml, m, box, k, nonsym):
    A = ml.problems.poisson_2d_5pt(m).tocsr().astype(np.float64)
    n = A.shape[0]
    if nonsym:  # a perturbation of the first superdiagonal only: A != A^T
        rng = np.random.default_rng(0)
        A = sp.csr_matrix(A + sp.diags([0.3 * rng.uniform(-1.0, 1.0, n - 1)], [1]))
        assert abs(A - A.T).max() > 0.01
    A.sort_indices()
    agg = sp.csr_matrix(ml.problems.box_aggregates_2d(m, m, box))
    Dinv = sp.diags([1.0 / A.diagonal()], [0])
    P = sp.csr_matrix((sp.eye(n) - (2.0 / 3.0) * Dinv @ A) @ agg)
    P.sum_duplicates()
    P.sort_indices()
    X = np.random.RandomState(1000 + m).standard_normal((n, k))
    X = X / np.linalg.norm(X, 2, axis=0)
    return A, P, X


def reference_loss_and_grad(torch, A, P, X0, tot_num_loop, nu1, nu2):
    """ns/model/loss.py:48-96, dense, torch fp64 on the CPU; d loss / d P.data by autograd."""
    Ad = torch.tensor(A.toarray(), dtype=torch.float64)
    rows = torch.tensor(np.repeat(np.arange(P.shape[0]), np.diff(P.indptr)), dtype=torch.long)
    cols = torch.tensor(P.indices.astype(np.int64), dtype=torch.long)
    vals = torch.tensor(P.data, dtype=torch.float64, requires_grad=True)
    Pd = torch.zeros(P.shape, dtype=torch.float64).index_put((rows, cols), vals)
    Dinv = ((2.0 / 3.0) / torch.diagonal(Ad))[:, None]
    A_H = Pd.T @ Ad @ Pd
    x = torch.tensor(X0, dtype=torch.float64)
    errs = []
    for _ in range(tot_num_loop + 1):
        for _ in range(nu1):
            x = x - Dinv * (Ad @ x)
        r_H = Pd.T @ (Ad @ x)
        e_H = torch.linalg.solve(A_H, -r_H)
        x = x + Pd @ e_H
        for _ in range(nu2):
            x = x - Dinv * (Ad @ x)
        x = x - x.mean(0)
        errs.append(torch.linalg.vector_norm(x, ord=2, dim=0))
    convs = (errs[-1] / errs[-3]) ** (1 / 2)
    loss = torch.softmax(convs, dim=0) @ convs
    loss.backward()
    return float(loss.detach()), vals.grad.numpy().copy(), torch.stack(errs).detach().numpy()


@pytest.fixture(scope="module")
def cases(ml, torch_cuda):
    """Per problem: the operators, the device (loss, grad, convs, errs) and the CPU autograd
    reference, computed once and left unchanged."""
    out = {}
    for name, m, box, k, nu, nonsym in PROBLEMS:
        A, P, X = _problem(ml, m, box, k, nonsym)
        got = ml.loss.amg_loss_and_grad(P, A, X, TOT, nu[0], nu[1], return_factors=True)
        ref = reference_loss_and_grad(torch_cuda, A, P, X, TOT, nu[0], nu[1])
        out[name] = {"A": A, "P": P, "X": X, "nu": nu, "got": got, "ref": ref}
    return out


@pytest.mark.parametrize("name", NAMES)
def test_forward_history_is_bitwise_amg_loss(ml, cases, name):
    c = cases[name]
    loss, grad, convs, errs = c["got"]
    l0, c0, e0 = ml.loss.amg_loss(c["P"], c["A"], c["X"], TOT, c["nu"][0], c["nu"][1],
                                  return_factors=True)
    assert errs.shape == (TOT + 1, c["X"].shape[1]) and grad.shape == (c["P"].nnz,)
    assert grad.dtype == np.float64
    assert np.array_equal(errs, e0)
    assert np.array_equal(convs, c0) and loss == l0
    # the restated history agrees with the device's within the project's dense-solve bound
    assert np.allclose(errs, c["ref"][2], rtol=1e-10, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_matches_autograd(cases, name):
    c = cases[name]
    grad, ref = c["got"][1], c["ref"][1]
    rel = np.abs(grad - ref).max() / np.abs(ref).max()
    print(f"{name}: max|grad - ref| / max|ref| = {rel:.3e}  (max|ref| = {np.abs(ref).max():.3e}, "
          f"loss {c['got'][0]:.15f} ref {c['ref'][0]:.15f})")
    assert np.all(np.isfinite(grad))
    assert rel <= GRAD_RTOL, (name, rel)


@pytest.mark.parametrize("name", NAMES)
def test_finite_difference_of_the_existing_forward(ml, cases, name):
    """A central difference of amg_loss (none of the new code) along a seeded random unit
    direction against grad . d."""
    c = cases[name]
    A, P, X, nu = c["A"], c["P"], c["X"], c["nu"]
    d = np.random.RandomState(77).standard_normal(P.nnz)
    d /= np.linalg.norm(d)

    def f(t):
        Pt = sp.csr_matrix((P.data + t * d, P.indices, P.indptr), shape=P.shape)
        return ml.loss.amg_loss(Pt, A, X, TOT, nu[0], nu[1])

    fd = (f(FD_H) - f(-FD_H)) / (2.0 * FD_H)
    gd = float(c["got"][1] @ d)
    rel = abs(fd - gd) / abs(gd)
    print(f"{name}: fd {fd:.12e} grad.d {gd:.12e} rel {rel:.3e}")
    assert rel <= FD_RTOL, (name, fd, gd)


def test_autograd_surface(ml, torch_cuda, cases):
    torch = torch_cuda
    c = cases["poisson12_box3"]
    A, P, X, nu = c["A"], c["P"], c["X"], c["nu"]
    loss0, grad0 = c["got"][0], c["got"][1]
    for device in ("cuda", "cpu"):
        v = torch.tensor(P.data, dtype=torch.float64, device=device, requires_grad=True)
        out = ml.loss.amg_loss_values(v, P.indptr, P.indices, P.shape, A, X, TOT, *nu)
        assert out.ndim == 0 and out.dtype == torch.float64 and out.device == v.device
        assert out.grad_fn is not None and float(out.detach()) == loss0
        out.backward()
        assert v.grad.device == v.device
        assert np.array_equal(v.grad.cpu().numpy(), grad0), device
    v = torch.tensor(P.data, dtype=torch.float64, device="cuda", requires_grad=True)
    (3 * ml.loss.amg_loss_values(v, torch.as_tensor(P.indptr), torch.as_tensor(P.indices),
                                 P.shape, A, torch.as_tensor(X), TOT, *nu)).backward()
    assert np.array_equal(v.grad.cpu().numpy(), 3.0 * grad0)
    w = torch.tensor(P.data, dtype=torch.float64, device="cuda")
    plain = ml.loss.amg_loss_values(w, P.indptr, P.indices, P.shape, A, X, TOT, *nu)
    assert plain.grad_fn is None and not plain.requires_grad
    assert float(plain) == ml.loss.amg_loss(P, A, X, TOT, *nu)
    # other operator types: a coalesced torch COO P gives the gradient in P.values() order
    coo = P.tocoo()
    Pt = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data, P.shape).coalesce()
    assert np.array_equal(Pt.values().numpy(), P.data)
    l2, g2 = ml.loss.amg_loss_and_grad(Pt, ml.sparse.DeviceCSR.from_scipy(A), X, TOT, *nu)
    assert l2 == loss0 and np.array_equal(g2, grad0)


def test_descent_from_the_tentative_prolongator(ml, torch_cuda):
    """Backtracking along -grad from the unsmoothed aggregate prolongator of Poisson 16^2 / 4x4
    boxes must lower amg_loss: a sign or transpose error fails here whatever the magnitudes."""
    m, k = 16, 8
    A = ml.problems.poisson_2d_5pt(m).tocsr()
    P = sp.csr_matrix(ml.problems.box_aggregates_2d(m, m, 4), dtype=np.float64)
    P.sort_indices()
    X = np.random.RandomState(5).standard_normal((m * m, k))
    X = X / np.linalg.norm(X, 2, axis=0)
    loss, grad = ml.loss.amg_loss_and_grad(P, A, X)
    assert loss == ml.loss.amg_loss(P, A, X)
    t, found = 1.0, None
    for _ in range(21):
        Pt = sp.csr_matrix((P.data - t * grad, P.indices, P.indptr), shape=P.shape)
        lt = ml.loss.amg_loss(Pt, A, X)
        if lt < loss:
            found = (t, lt)
            break
        t *= 0.5
    print(f"descent: loss {loss:.6f} -> {found}")
    assert found is not None


def test_gradient_is_deterministic(ml, cases):
    c = cases["nonsym12_box3"]
    l2, g2 = ml.loss.amg_loss_and_grad(c["P"], c["A"], c["X"], TOT, *c["nu"])
    assert l2 == c["got"][0] and np.array_equal(g2, c["got"][1])


def test_refusals(ml, torch_cuda, cases):
    torch = torch_cuda
    c = cases["poisson12_box3"]
    A, P, X = c["A"], c["P"], c["X"]
    with pytest.raises(NotImplementedError, match="neumann_solve_fix"):
        ml.loss.amg_loss_and_grad(P, A, X, neumann_solve_fix=True)
    # unsorted column indices within a row
    idx = P.indices.copy()
    r = int(np.argmax(np.diff(P.indptr) >= 2))
    a = P.indptr[r]
    idx[a], idx[a + 1] = idx[a + 1], idx[a]
    bad = sp.csr_matrix((P.data, idx, P.indptr), shape=P.shape)
    with pytest.raises(ValueError, match="canonical"):
        ml.loss.amg_loss_and_grad(bad, A, X)
    with pytest.raises(ValueError, match="canonical"):
        ml.loss.amg_loss_and_grad(ml.sparse.DeviceCSR.from_scipy(bad, check=False), A, X)
    Xg = torch.tensor(X, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="test_vecs"):
        ml.loss.amg_loss_and_grad(P, A, Xg)
    v = torch.tensor(P.data, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="test_vecs"):
        ml.loss.amg_loss_values(v, P.indptr, P.indices, P.shape, A, Xg)
    At = torch.sparse_coo_tensor(np.vstack(A.nonzero()), A.tocoo().data, A.shape,
                                 requires_grad=True)
    with pytest.raises(NotImplementedError, match="A requires grad"):
        ml.loss.amg_loss_values(v, P.indptr, P.indices, P.shape, At, X)
    with pytest.raises(ValueError, match="1 to 64"):
        ml.loss.amg_loss_and_grad(P, A, np.ones((A.shape[0], 65)))
    with pytest.raises(ValueError, match="tot_num_loop"):
        ml.loss.amg_loss_and_grad(P, A, X, tot_num_loop=1)
