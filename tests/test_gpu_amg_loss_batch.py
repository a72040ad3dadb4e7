"""GPU: amg_loss and its gradient over a batch of problems (mlamg.loss.AmgLossBatch, DESIGN.md
§24). Problem i's error history, convergence factors, loss and gradient are bitwise what
amg_loss_and_grad(P_i, A_i, X_i, ...) returns.

The independent reference is `reference_loss_and_grad` below: ns/model/loss.py:48-96 restated
densely in torch fp64 on the CPU, one problem at a time, with torch.linalg.solve for the coarse
system and .backward(). Nothing of the library runs in it. The gradient bound is GRAD_RTOL of
tests/test_gpu_amg_loss_grad.py (100 x the worst 6.3e-15 measured there, never above 1e-9), the
history agrees at rtol 1e-10.

Measured on the MI355X (printed by test_batch_matches_autograd),
max |grad - ref| / max |ref|: 8.0e-16 (Poisson 6^2), 1.7e-15 (9^2), 2.4e-15 (12^2), 1.0e-14
(24^2), 3.3e-15 (non-symmetric 27^2), 1.6e-15 (Poisson 16^2, nu = (2, 2)); the bound is 6.3e-13."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

WORST_MEASURED = 6.3e-15  # tests/test_gpu_amg_loss_grad.py
GRAD_RTOL = min(100.0 * WORST_MEASURED, 1e-9)
TOT, K = 5, 4

#           m  box  non-symmetric
MIXED = ((6, 3, False), (9, 3, False), (12, 3, False), (24, 3, False), (27, 3, True))
SYMMETRIC = ((6, 3, False), (9, 3, False), (12, 3, False), (24, 3, False))


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
    """tests/test_gpu_amg_loss_grad.py's problem: Poisson m^2 (with that file's superdiagonal
    perturbation when nonsym), box aggregates, the Jacobi-smoothed P, seeded unit test vectors."""
    A = ml.problems.poisson_2d_5pt(m).tocsr().astype(np.float64)
    n = A.shape[0]
    if nonsym:
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


def _batch_case(ml, torch, spec, nu):
    """One batch: the problems, the batch object and its result, the single calls and the CPU
    autograd reference per problem."""
    probs = [_problem(ml, m, box, K, nonsym) for m, box, nonsym in spec]
    As, Ps, Xs = (list(t) for t in zip(*probs))
    B = ml.loss.AmgLossBatch(As, Ps, Xs, TOT, nu[0], nu[1])
    values = np.concatenate([P.data for P in Ps])
    got = B.loss_and_grad(values, return_factors=True)
    single = [ml.loss.amg_loss_and_grad(P, A, X, TOT, nu[0], nu[1], return_factors=True)
              for A, P, X in probs]
    ref = [reference_loss_and_grad(torch, A, P, X, TOT, nu[0], nu[1]) for A, P, X in probs]
    return {"probs": probs, "B": B, "values": values, "got": got, "single": single, "ref": ref}


@pytest.fixture(scope="module")
def cases(ml, torch_cuda):
    """Computed once and left unchanged: the mixed batch (its last problem makes the stack
    non-symmetric: the second block inverse), the all-symmetric V(1,1) batch and Poisson 16^2
    with 4 x 4 boxes and V(2,2) (a batch of one problem)."""
    return {"mixed": _batch_case(ml, torch_cuda, MIXED, (1, 1)),
            "symmetric": _batch_case(ml, torch_cuda, SYMMETRIC, (1, 1)),
            "poisson16_nu22": _batch_case(ml, torch_cuda, ((16, 4, False),), (2, 2))}


NAMES = ("mixed", "symmetric", "poisson16_nu22")


@pytest.mark.parametrize("name", NAMES)
def test_batch_is_bitwise_the_single_calls(cases, name):
    c = cases[name]
    losses, grad, convs, errs = c["got"]
    B, nb = c["B"], len(c["probs"])
    assert B.symmetric == (name != "mixed")
    assert losses.shape == (nb,) and convs.shape == (nb, K) and errs.shape == (TOT + 1, nb, K)
    assert grad.shape == (int(B.nnz_offsets[-1]),) and grad.dtype == np.float64
    for i, (l1, g1, c1, e1) in enumerate(c["single"]):
        a, b = int(B.nnz_offsets[i]), int(B.nnz_offsets[i + 1])
        assert np.array_equal(errs[:, i, :], e1), i
        assert np.array_equal(convs[i], c1), i
        assert losses[i] == l1, i
        assert np.array_equal(grad[a:b], g1), i


@pytest.mark.parametrize("name", NAMES)
def test_batch_matches_autograd(cases, name):
    c = cases[name]
    losses, grad, convs, errs = c["got"]
    B = c["B"]
    worst = 0.0
    for i, (l0, g0, e0) in enumerate(c["ref"]):
        a, b = int(B.nnz_offsets[i]), int(B.nnz_offsets[i + 1])
        rel = np.abs(grad[a:b] - g0).max() / np.abs(g0).max()
        worst = max(worst, rel)
        print(f"{name}[{i}] n = {c['probs'][i][0].shape[0]}: max|grad - ref| / max|ref| = "
              f"{rel:.3e}, loss {losses[i]:.15f} ref {l0:.15f}")
        assert np.all(np.isfinite(grad[a:b]))
        assert rel <= GRAD_RTOL, (name, i, rel)
        assert np.allclose(errs[:, i, :], e0, rtol=1e-10, atol=0), (name, i)
    print(f"{name}: worst {worst:.3e} (bound {GRAD_RTOL:.1e})")


def test_autograd_surface(ml, torch_cuda, cases):
    torch = torch_cuda
    c = cases["mixed"]
    B, nb = c["B"], len(c["probs"])
    losses0, grad0 = c["got"][0], c["got"][1]
    for device in ("cuda", "cpu"):
        v = torch.tensor(c["values"], dtype=torch.float64, device=device, requires_grad=True)
        out = B.loss_values(v)
        assert out.shape == (nb,) and out.dtype == torch.float64 and out.device == v.device
        assert out.grad_fn is not None
        assert np.array_equal(out.detach().cpu().numpy(), losses0)
        out.sum().backward()
        assert v.grad.device == v.device
        assert np.array_equal(v.grad.cpu().numpy(), grad0), device
        with pytest.raises(RuntimeError):  # the saved gradient is gone: no second backward
            out.sum().backward()
    v = torch.tensor(c["values"], dtype=torch.float64, device="cuda", requires_grad=True)
    B.loss_values(v).mean().backward()
    w = torch.full((nb,), 1.0 / nb, dtype=torch.float64)  # mean()'s grad_output
    seg = torch.as_tensor(np.repeat(np.arange(nb), np.diff(B.nnz_offsets)))
    assert np.array_equal(v.grad.cpu().numpy(), grad0 * w[seg].numpy())
    plain = B.loss_values(torch.tensor(c["values"], dtype=torch.float64, device="cuda"))
    assert plain.grad_fn is None and np.array_equal(plain.cpu().numpy(), losses0)
    # values as a list of per-problem arrays; the forward-only entry
    l2, g2 = B.loss_and_grad([P.data for _, P, _ in c["probs"]])
    assert np.array_equal(l2, losses0) and np.array_equal(g2, grad0)
    assert np.array_equal(B.loss(c["values"]), losses0)


def test_second_backward_raises(torch_cuda, cases):
    torch = torch_cuda
    c = cases["symmetric"]
    v = torch.tensor(c["values"], dtype=torch.float64, device="cuda", requires_grad=True)
    out = c["B"].loss_values(v).sum()
    (g,) = torch.autograd.grad(out, v, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_repeatable_and_problems_are_independent(cases):
    c = cases["mixed"]
    B = c["B"]
    losses0, grad0, convs0, errs0 = c["got"]
    l1, g1, c1, e1 = B.loss_and_grad(c["values"], return_factors=True)
    assert np.array_equal(l1, losses0) and np.array_equal(g1, grad0)
    assert np.array_equal(c1, convs0) and np.array_equal(e1, errs0)
    # other values for problem 2 only: nothing of the other problems changes by a bit
    a, b = int(B.nnz_offsets[2]), int(B.nnz_offsets[3])
    v = c["values"].copy()
    v[a:b] *= 1.0 + 0.05 * np.cos(np.arange(b - a))
    l2, g2, _, e2 = B.loss_and_grad(v, return_factors=True)
    others = np.array([i for i in range(len(losses0)) if i != 2])
    assert l2[2] != losses0[2] and not np.array_equal(g2[a:b], grad0[a:b])
    assert np.array_equal(l2[others], losses0[others])
    assert np.array_equal(e2[:, others, :], errs0[:, others, :])
    assert np.array_equal(g2[:a], grad0[:a]) and np.array_equal(g2[b:], grad0[b:])


def test_convenience_wrappers_and_generated_test_vectors(ml, cases):
    """test_vecs = k: problem i gets what amg_loss(P_i, A_i, k) generates."""
    probs = cases["symmetric"]["probs"][:3]
    As, Ps = [p[0] for p in probs], [p[1] for p in probs]
    losses, grad = ml.loss.amg_loss_and_grad_batch(Ps, As, 3)
    only = ml.loss.amg_loss_batch(Ps, As, 3)
    off = np.concatenate([[0], np.cumsum([P.nnz for P in Ps])])
    for i, (A, P) in enumerate(zip(As, Ps)):
        l1, g1 = ml.loss.amg_loss_and_grad(P, A, 3)
        assert losses[i] == l1 == only[i] == ml.loss.amg_loss(P, A, 3)
        assert np.array_equal(grad[off[i]:off[i + 1]], g1)


def test_adam_on_the_mean_loss_descends(ml, torch_cuda):
    """A few Adam steps on losses.mean() from the tentative prolongators of three grids."""
    torch = torch_cuda
    As, Ps = [], []
    for m in (8, 12, 16):
        As.append(ml.problems.poisson_2d_5pt(m).tocsr())
        P = sp.csr_matrix(ml.problems.box_aggregates_2d(m, m, 4), dtype=np.float64)
        P.sort_indices()
        Ps.append(P)
    B = ml.loss.AmgLossBatch(As, Ps, 8)
    v = torch.tensor(np.concatenate([P.data for P in Ps]), dtype=torch.float64, device="cuda",
                     requires_grad=True)
    opt = torch.optim.Adam([v], lr=0.02)
    hist = []
    for _ in range(6):
        opt.zero_grad()
        loss = B.loss_values(v).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    hist.append(float(B.loss_values(v.detach()).mean()))
    print("mean loss per Adam step:", " ".join(f"{h:.6f}" for h in hist))
    assert hist[-1] < hist[0]
