"""GPU: the block PCG coarse solve (mlamg_pcg_solve_mv, csrc/pcg.hip) and what it
lifts the dense-only cap from: the block cycle (Hierarchy.cycle_multi, precondition on a block),
amg_loss and its gradient with respect to P.

The contract is §17's, extended to PCG: column j of every block result, and column j's iteration
count, are bitwise the single-vector result on column j. Small PCG hierarchies with a real inner
hierarchy are forced as tests/test_gpu_coarse_pcg.py forces them: TWO_LEVEL_DENSE_MAX and
PCG_INNER_MAX_COARSE patched down on poisson_2d_5pt(48) with the device's SA prolongator
(alpha = 0.1, n_c ~ 230). All comparisons are np.array_equal unless a tolerance is stated.

The gradient's tolerance. Measured on the MI355X (printed by test_gradient_with_pcg_coarse),
max |grad - ref| / max |ref| of the PCG-coarse gradient:
  against the torch fp64 CPU autograd reference   5.82e-13 (amg_loss_and_grad and the autograd
                                                  surface amg_loss_values(...).backward() alike)
  against the dense-coarse device gradient        5.88e-13
(the dense-coarse gradient itself: 9.6e-15 from the reference).
The coarse solves stop at a relative residual of 1e-12 and the adjoint treats them as exact, so
the expected error is of the order 1e-12 * cond(A_H) with cond(A_H) in the hundreds on this grid;
the assertion is 100 times the worst measured value (5.9e-11) and never above 1e-8, beyond which
the difference would be a defect to investigate, not a tolerance to widen."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

M = 48           # grid: 2,304 rows
CYCLES = 4
TOT = 5          # amg_loss cycles - 1
WORST_MEASURED = 5.9e-13
GRAD_RTOL = min(100.0 * WORST_MEASURED, 1e-8)


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
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def problem(ml):
    """A, the canonical SA prolongator of the device's first level, and k = 4 test vectors."""
    A = ml.problems.poisson_2d_5pt(M).tocsr().astype(np.float64)
    A.sort_indices()
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_levels=2, finalize=False)
    P = sp.csr_matrix(H.levels[0].P.to_scipy(), dtype=np.float64)
    P.sum_duplicates()
    P.sort_indices()
    assert 150 <= P.shape[1] <= 400
    X = np.random.RandomState(11).standard_normal((A.shape[0], 4))
    X = X / np.linalg.norm(X, 2, axis=0)
    return A, P, X


def _force_pcg(monkeypatch, ml):
    H_ = ml.hierarchy.Hierarchy
    monkeypatch.setattr(H_, "TWO_LEVEL_DENSE_MAX", 16)
    monkeypatch.setattr(H_, "PCG_INNER_MAX_COARSE", 60)


def _pcg_two_level(ml, A, P, **kw):
    H = ml.hierarchy.Hierarchy.two_level(A, P, **kw)
    assert H.pcg is not None and H.inner.n_levels >= 2
    return H


def _stats(H):
    st = H.coarse_stats()
    return st["total_iters"], st["not_converged"], st["max_rel_residual"], st["breakdowns"]


def _rhs(Ac, k):
    """k right-hand sides of A_c: random, zero, a smooth mode (one more iteration than the random
    column on the MI355X: 14, 0, 15), A_c @ ones, scaled random, a unit vector and more random
    columns."""
    n = Ac.shape[0]
    rs = np.random.RandomState(21)
    t = np.arange(n) / n
    cols = [rs.standard_normal(n), np.zeros(n), np.sin(np.pi * t), Ac @ np.ones(n),
            1e-3 * rs.standard_normal(n), np.eye(n)[:, n // 2]]
    while len(cols) < k:
        cols.append(rs.standard_normal(n))
    return np.stack(cols[:k], axis=1)


@pytest.fixture(scope="module")
def single_solves(ml, torch_cuda, problem):
    """mlamg_pcg_solve on each of 9 columns, one after the other on one freshly built solver: per
    column x, the iteration count and the solver's cumulative statistics after that solve."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    A, P, _ = problem
    with pytest.MonkeyPatch.context() as mp:
        _force_pcg(mp, ml)
        H = _pcg_two_level(ml, A, P)
    Ac = H.Ac.to_scipy()
    B = _rhs(Ac, 9)
    out = []
    for j in range(B.shape[1]):
        b = dev(torch, B[:, j])
        x = torch.full_like(b, np.nan)
        call("mlamg_pcg_solve", H.pcg, ptr(b), ptr(x), stream_ptr())
        st = H.coarse_stats()
        out.append({"x": host(x), "iters": st["last_iters"], "stats": _stats(H)})
    its = sorted({o["iters"] for o in out[:3]} - {0})
    assert len(its) >= 2, [o["iters"] for o in out]  # freezing runs while other columns go on
    assert out[1]["iters"] == 0 and not out[1]["x"].any()
    return Ac, B, out


def _block_solve(torch, H, Bd, Xd, k):
    from mlamg._lib import call, ptr, stream_ptr
    call("mlamg_pcg_solve_mv", H.pcg, ptr(Bd), Bd.stride(0), ptr(Xd), Xd.stride(0), k,
         stream_ptr())
    it = (ctypes.c_int32 * k)()
    call("mlamg_pcg_iters_mv", H.pcg, it, k, stream_ptr())
    return list(it)


@pytest.mark.parametrize("k", (1, 3, 8, 9))
def test_columns_are_bitwise_the_single_solve(ml, torch_cuda, problem, single_solves,
                                              monkeypatch, k):
    torch = torch_cuda
    A, P, _ = problem
    Ac, B, ref = single_solves
    _force_pcg(monkeypatch, ml)
    H = _pcg_two_level(ml, A, P)
    Bd = dev(torch, B[:, :k])
    Xd = torch.full((Ac.shape[0], k), np.nan, dtype=torch.float64, device="cuda")
    iters = _block_solve(torch, H, Bd, Xd, k)
    X = host(Xd)
    print(f"k = {k}: iterations {iters}")
    for j in range(k):
        assert iters[j] == ref[j]["iters"], (j, iters, [r["iters"] for r in ref[:k]])
        assert np.array_equal(X[:, j], ref[j]["x"]), j
        b = B[:, j]
        assert np.linalg.norm(b - Ac @ X[:, j]) <= 1.01e-12 * np.linalg.norm(b), j
    # the statistics read as after k single solves
    assert _stats(H) == ref[k - 1]["stats"]
    assert H.coarse_stats()["last_iters"] == ref[k - 1]["iters"]
    total, not_conv, rel, brk = _stats(H)
    assert total == sum(r["iters"] for r in ref[:k]) and not_conv == 0 and brk == 0
    assert rel <= 1e-12
    # a second solve on the same solver gives the same bits (stale work blocks do not matter)
    Xd.fill_(np.nan)
    assert _block_solve(torch, H, Bd, Xd, k) == iters and np.array_equal(host(Xd), X)


def test_column_slices_of_wider_blocks(ml, torch_cuda, problem, single_solves, monkeypatch):
    """ld > k, odd column offsets (8-byte aligned pointers only): columns 0..4 of the right-hand
    sides sit in columns 3..7 of a 12-wide block, the result in columns 1..5 of a 13-wide one,
    whose other columns stay untouched."""
    torch = torch_cuda
    A, P, _ = problem
    Ac, B, ref = single_solves
    _force_pcg(monkeypatch, ml)
    H = _pcg_two_level(ml, A, P)
    n, k = Ac.shape[0], 5
    Bw = torch.full((n, 12), 5.0, dtype=torch.float64, device="cuda")
    Xw = torch.full((n, 13), 7.0, dtype=torch.float64, device="cuda")
    Bw[:, 3:3 + k] = dev(torch, B[:, :k])
    iters = _block_solve(torch, H, Bw[:, 3:3 + k], Xw[:, 1:1 + k], k)
    Xh = host(Xw)
    assert iters == [r["iters"] for r in ref[:k]]
    for j in range(k):
        assert np.array_equal(Xh[:, 1 + j], ref[j]["x"]), j
    assert np.all(Xh[:, 0] == 7.0) and np.all(Xh[:, 1 + k:] == 7.0)
    assert np.all(host(Bw)[:, :3] == 5.0) and np.all(host(Bw)[:, 3 + k:] == 5.0)
    assert _stats(H) == ref[k - 1]["stats"]


def test_block_cycle_with_pcg_coarse(ml, torch_cuda, problem, monkeypatch):
    """cycle_multi on a two-level hierarchy with a PCG coarse solve: X and the history are
    bitwise the single-vector cycle per column (the comparison of the dense-coarse case,
    tests/test_gpu_multivector.py, its definition of the history included)."""
    torch = torch_cuda
    from test_gpu_multivector import _single_loop
    A, P, _ = problem
    _force_pcg(monkeypatch, ml)
    H = _pcg_two_level(ml, A, P)
    n, k = A.shape[0], 5
    rs = np.random.RandomState(7)
    X0 = dev(torch, rs.standard_normal((n, k)))
    B = dev(torch, rs.standard_normal((n, k)))
    for norm, remove_mean, Bm in (("residual", False, B), ("x", True, None)):
        X = X0.clone()
        hist = H.cycle_multi(Bm, X, CYCLES, norm=norm, remove_mean=remove_mean)
        assert hist.shape == (CYCLES, k)
        for j in range(k):
            xj = X0[:, j].contiguous()
            bj = Bm[:, j].contiguous() if Bm is not None else None
            hj = _single_loop(torch, H, bj, xj, CYCLES, norm, remove_mean)
            assert np.array_equal(host(X[:, j]), host(xj)), (norm, j)
            assert np.array_equal(hist[:, j], hj), (norm, j, hist[:, j], hj)
    st = H.coarse_stats()
    assert st["not_converged"] == 0 and st["breakdowns"] == 0 and st["max_rel_residual"] <= 1e-12
    Z = H.precondition(B)
    for j in range(k):
        assert np.array_equal(host(Z[:, j]), host(H.precondition(B[:, j].contiguous()))), j


@pytest.fixture(scope="module")
def loss_cases(ml, torch_cuda, problem):
    """amg_loss and its gradient with the PCG coarse solve (patched) and with the dense one, and
    the CPU autograd reference: computed once."""
    from test_gpu_amg_loss_grad import reference_loss_and_grad
    A, P, X = problem
    out = {"dense": ml.loss.amg_loss(P, A, X, TOT, return_factors=True),
           "dense_grad": ml.loss.amg_loss_and_grad(P, A, X, TOT, return_factors=True),
           "ref": reference_loss_and_grad(torch_cuda, A, P, X, TOT, 1, 1)}
    with pytest.MonkeyPatch.context() as mp:
        _force_pcg(mp, ml)
        out["H"] = _pcg_two_level(ml, A, P, omega=2.0 / 3.0)
        out["pcg"] = ml.loss.amg_loss(P, A, X, TOT, return_factors=True)
        out["pcg_grad"] = ml.loss.amg_loss_and_grad(P, A, X, TOT, return_factors=True)
        v = torch_cuda.tensor(P.data, dtype=torch_cuda.float64, device="cuda",
                              requires_grad=True)
        loss = ml.loss.amg_loss_values(v, P.indptr, P.indices, P.shape, A, X, TOT)
        loss.backward()
        out["autograd"] = (float(loss.detach()), v.grad.cpu().numpy())
    return out


def test_amg_loss_pcg_against_dense(ml, torch_cuda, problem, loss_cases):
    """The PCG-coarse history against the dense-coarse one within the project's
    SuperLU-versus-dense bounds (errs rtol 1e-10, convs 1e-8; tests/test_gpu_coarse_pcg.py,
    SURVEY.md §8(d)), and bitwise against the single-vector loop."""
    torch = torch_cuda
    from test_gpu_multivector import _single_loop
    A, P, X = problem
    loss_d, convs_d, errs_d = loss_cases["dense"]
    loss_p, convs_p, errs_p = loss_cases["pcg"]
    assert errs_p.shape == (TOT + 1, X.shape[1])
    assert not np.array_equal(errs_p, errs_d)  # another coarse solver did run
    assert np.allclose(errs_p, errs_d, rtol=1e-10, atol=0), (errs_p, errs_d)
    assert np.abs(convs_p - convs_d).max() <= 1e-8 and abs(loss_p - loss_d) <= 1e-8
    H = loss_cases["H"]
    for j in range(X.shape[1]):
        xj = dev(torch, X[:, j])
        assert np.array_equal(errs_p[:, j], _single_loop(torch, H, None, xj, TOT + 1, "x", True)), j


def test_gradient_with_pcg_coarse(problem, loss_cases):
    A, P, X = problem
    loss, grad, convs, errs = loss_cases["pcg_grad"]
    assert np.array_equal(errs, loss_cases["pcg"][2]) and loss == loss_cases["pcg"][0]
    assert np.array_equal(convs, loss_cases["pcg"][1])
    assert grad.shape == (P.nnz,) and np.all(np.isfinite(grad))
    ref = loss_cases["ref"][1]
    dense = loss_cases["dense_grad"][1]
    auto_loss, auto_grad = loss_cases["autograd"]
    assert auto_loss == loss
    rels = {"grad vs autograd ref": np.abs(grad - ref).max() / np.abs(ref).max(),
            "values.backward vs autograd ref": np.abs(auto_grad - ref).max() / np.abs(ref).max(),
            "grad vs dense-coarse grad": np.abs(grad - dense).max() / np.abs(dense).max(),
            "values.backward vs dense-coarse grad":
                np.abs(auto_grad - dense).max() / np.abs(dense).max(),
            "dense-coarse grad vs autograd ref": np.abs(dense - ref).max() / np.abs(ref).max()}
    for name, rel in rels.items():
        print(f"{name}: max|a - b| / max|b| = {rel:.3e}")
    for name, rel in rels.items():
        assert rel <= GRAD_RTOL, (name, rel)


def test_still_refused(ml, torch_cuda, problem, monkeypatch):
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    A, P, X = problem
    H = ml.hierarchy.Hierarchy.two_level(A, P, coarse="gmres")
    assert H.coarse_gmres
    with pytest.raises(MlamgError, match="GMRES") as ei:
        H.cycle_multi(None, dev(torch, X), 1)
    assert ei.value.code == MLAMG_EUNSUPPORTED
    with pytest.raises(NotImplementedError, match="neumann_solve_fix"):
        ml.loss.amg_loss_and_grad(P, A, X, neumann_solve_fix=True)
    with pytest.raises(NotImplementedError, match="neumann_solve_fix"):
        ml.loss.amg_loss(P, A, X, neumann_solve_fix=True)
    # a coarse operator that is not symmetric, beyond the (patched) dense limits: GMRES
    n = A.shape[0]
    An = sp.csr_matrix(A + 0.5 * (sp.eye(n) - sp.eye(n, k=-1)))
    An.sort_indices()
    H_ = ml.hierarchy.Hierarchy
    monkeypatch.setattr(H_, "TWO_LEVEL_DENSE_MAX", 16)
    monkeypatch.setattr(H_, "DENSE_LIMIT", 64)
    monkeypatch.setattr(H_, "PCG_INNER_MAX_COARSE", 60)
    assert H_.two_level(An, P).coarse_gmres
    with pytest.raises(NotImplementedError, match="GMRES"):
        ml.loss.amg_loss_and_grad(P, An, X)
    v = torch.tensor(P.data, dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="GMRES"):
        ml.loss.amg_loss_values(v, P.indptr, P.indices, P.shape, An, X)


def test_breakdown_raises(ml, torch_cuda, monkeypatch):
    """The indefinite tridiag(1, 1, 1), n = 20,000, P = I of test_pcg_breakdown_is_reported: the
    block cycle's PCG breaks down in every column (a numerical stop, counted per column), and
    cycle_multi raises CoarseSolveError as cycle() does."""
    torch = torch_cuda
    H_ = ml.hierarchy.Hierarchy
    n, k = 20000, 3
    A = sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1], format="csr")
    P = sp.eye(n, format="csr")
    monkeypatch.setattr(H_, "TWO_LEVEL_DENSE_MAX", 64)
    H = H_.two_level(A, P, smoother="jacobi")
    assert H.pcg is not None
    B = dev(torch, np.random.RandomState(1).standard_normal((n, k)))
    X = torch.zeros((n, k), dtype=torch.float64, device="cuda")
    with pytest.raises(ml.hierarchy.CoarseSolveError):
        H.cycle_multi(B, X, 2)
    assert H.coarse_stats()["breakdowns"] >= 1
    with pytest.raises(ml.hierarchy.CoarseSolveError):
        H.precondition(B)
