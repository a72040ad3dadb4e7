"""lambda_max(D^-1 A) on the CPU: the algorithm of csrc/eig.hip, restated in numpy
(tests/lanczos_model.py), meets the project's bound of 1e-12 on every matrix that
tests/test_gpu_lambda_max.py holds the device to; so does the reference's own ARPACK call; and
the fp64 reference that referees both is itself checked against closed forms and a 50-digit
eigensolve. No kernel runs here."""
import numpy as np
import pytest

import lanczos_model as lm
from lanczos_model import BOUND

SEEDS = (0, 1, 2, 3)


# ---------------------------------------------------------------- the reference's own error
@pytest.mark.parametrize("name", sorted(lm.POISSON_1D))
def test_reference_vs_closed_form(name):
    exact = lm.poisson_closed_form(lm.POISSON_1D[name])
    assert abs(lm.reference(name) - exact) <= 1e-14 * exact


def test_reference_vs_50_digits():
    """The n = 64 jump matrix, whose top eigenvalues are the closest of the tridiagonal cases:
    LAPACK in fp64 is within 1e-14 of the 50-digit value, 100 times inside the bound."""
    exact = lm.reference_mp(lm.matrix("jump1d_64"), digits=50)
    assert abs(lm.reference("jump1d_64") - exact) <= 1e-14 * exact


def test_top_cluster_is_a_cluster():
    import scipy.linalg
    ev = scipy.linalg.eigvalsh(lm.scaled_dense(lm.matrix("top_cluster_200")))
    assert np.allclose(ev[-1] - ev[-3:], [1e-6, 5e-7, 0.0], rtol=0, atol=1e-12) and ev[-4] < 1.9


def test_galerkin_levels_have_dense_rows():
    for h in ("p2d48", "jump2d48", "jump1d150"):
        L = lm.galerkin_levels(h)
        width = [int(np.diff(A.indptr).max()) for A in L]
        assert [A.shape[0] for A in L] == ([2304, 256, 36] if h != "jump1d150" else [150, 50, 17])
        if h != "jump1d150":  # 9-point and wider coarse stencils; 1D stays tridiagonal
            assert width[0] == 5 and min(width[1:]) >= 9, (h, width)


# ---------------------------------------------------------------- the algorithm
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_model_meets_bound(name):
    A, ref = lm.matrix(name), lm.reference(name)
    for seed in SEEDS:
        lam, iters, _, _, m = lm.lanczos(A, seed=seed)
        assert abs(lam - ref) <= BOUND * ref, (name, seed, lam, ref, iters)
        assert iters % lm.CHECK == 0 and m <= iters
        if name in lm.TINY or name == "diagonal_40":  # ended by breakdown, at the first read
            want_m = 1 if name == "diagonal_40" else lm.POISSON_1D[name]
            assert (iters, m) == (lm.CHECK, want_m), (name, seed, iters, m)


@pytest.mark.parametrize("name,steps", (("jump1d_64", 160), ("jump1d_150", 480)))
def test_jump_cases_need_more_than_n_steps(name, steps):
    """What the cap at n steps cost (max_iter = n is that cap): seven and six orders of
    magnitude outside the bound, so these two cases tell a capped routine from this one."""
    A, ref = lm.matrix(name), lm.reference(name)
    n = A.shape[0]
    lam, iters, *_ = lm.lanczos(A, max_iter=n)
    assert iters == n and 1e-7 < abs(lam - ref) / ref < 1e-4, (lam, ref)
    assert lm.lanczos(A)[1] == steps > n


@pytest.mark.parametrize("name", ("jump1d_64", "jump1d_150", "poisson1d_2000", "galerkin_p2d48_L0",
                                  "galerkin_jump2d48_L1", "top_cluster_200"))
def test_loose_tolerances(name):
    """The tolerances mlamg/hierarchy.py passes: the Ritz value stays below lambda_max (up to
    rounding) and the steps do not grow as tol loosens. No lower bound: the stop test is a
    stagnation test."""
    A, ref = lm.matrix(name), lm.reference(name)
    its = []
    for tol in (1e-15, 1e-8, 1e-6):
        lam, iters, *_ = lm.lanczos(A, tol=tol)
        assert lam <= ref * (1 + BOUND), (name, tol, lam, ref)
        its.append(iters)
    assert its[0] >= its[1] >= its[2], its


@pytest.mark.parametrize("kind", sorted(lm.BAD_DIAGONALS))
def test_bad_diagonals_raise(kind):
    A = lm.BAD_DIAGONALS[kind](lm.poisson_1d(40))
    if kind == "zero":  # stored, and zero
        assert A.nnz == lm.poisson_1d(40).nnz and A.diagonal()[37] == 0.0
    if kind == "missing":
        assert A.nnz == lm.poisson_1d(40).nnz - 1
    with pytest.raises(lm.BadDiagonal):
        lm.lanczos(A)


def test_start_vector_matches_the_distributed_restatement():
    from mlamg import dsetup
    for seed in SEEDS:
        assert np.array_equal(lm.splitmix_start(300, seed), dsetup._splitmix_start(0, 300, seed))
        assert np.array_equal(lm.splitmix_start(300, seed)[100:],
                              dsetup._splitmix_start(100, 300, seed))


# ---------------------------------------------------------------- the reference pipeline
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_arpack_within_bound(oracle, name):
    """The reference's own call (ARPACK eigs on D^-1 A, oracle.arpack_lambda_max) converges and
    is inside the bound on every case the device is held to: the bound is one that the pipeline
    being reproduced keeps. At n = 1 and n = 2 scipy's eigs has no ARPACK path (k = 1 >= n - 1
    on a sparse operator is a TypeError), so the reference has no value there; those two cases
    are held to the closed form alone."""
    A, ref = lm.matrix(name), lm.reference(name)
    if A.shape[0] <= 2:
        with pytest.raises(TypeError):
            oracle.arpack_lambda_max(A)
        return
    lam = oracle.arpack_lambda_max(A)  # ArpackNoConvergence would raise
    assert abs(lam - ref) <= BOUND * ref, (name, lam, ref)
