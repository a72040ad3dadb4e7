"""CPU: the Chebyshev coefficients (pyamg.relaxation.chebyshev restated) and the host model of the
polynomial sweep that the GPU tests compare against (tests/poly_model.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import poly_model
from mlamg.pyamg_compat.relaxation.chebyshev import chebyshev_polynomial_coefficients


@pytest.mark.parametrize("a,b", [(1.0 / 30.0, 1.1), (0.2, 7.5), (3.0, 3.5)])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 6])
def test_coefficients_are_the_scaled_chebyshev_polynomial(a, b, degree):
    p = chebyshev_polynomial_coefficients(a, b, degree)
    assert p.shape == (degree + 1,)
    assert abs(np.polyval(p, 0.0) - 1.0) <= 1e-14
    assert p[-1] == pytest.approx(1.0, abs=1e-14)
    roots = 0.5 * (b - a) * (1 + np.cos(np.pi * (np.arange(degree) + 0.5) / degree)) + a
    # Horner's |p|(|x|) bounds each evaluation's rounding; the issue's bound is 1e-12 max|p|
    assert np.all(np.abs(np.polyval(p, roots)) <= 1e-12 * np.abs(p).max())


def test_degree_one_closed_form():
    for a, b in ((1.0 / 30.0, 1.1), (0.5, 2.0), (1e-3, 40.0)):
        p = chebyshev_polynomial_coefficients(a, b, 1)
        want = np.array([-2.0 / (a + b), 1.0])
        assert np.all(np.abs(p - want) <= 2 * np.spacing(np.abs(want)))


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (2.0, 1.0), (0.0, 1.0), (-0.5, 1.0)])
def test_invalid_intervals_raise(a, b):
    with pytest.raises(ValueError):
        chebyshev_polynomial_coefficients(a, b, 3)


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.linspace(0.05, 2.0, n)
    return (Q * lam) @ Q.T, Q, lam


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sweep_applies_p_of_A_to_the_error(degree):
    """With b = 0 one sweep with -p[:-1] maps e to p(A) e: pins that c[0] multiplies the highest
    power (pyamg's order). Compared through A's eigendecomposition."""
    M, Q, lam = _spd(12, 3)
    M = 0.5 * (M + M.T)
    A = sp.csr_matrix(M)
    p = chebyshev_polynomial_coefficients(lam[0], 1.1 * lam[-1], degree)
    e = np.random.default_rng(4).standard_normal(12)
    got = poly_model.sweep(A, e, None, -p[:-1])
    want = Q @ (np.polyval(p, lam) * (Q.T @ e))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_zero_guess_model_is_the_general_model_on_zero(m):
    rng = np.random.default_rng(m)
    A = sp.random(40, 40, density=0.15, random_state=rng, format="csr")
    A.data[:] = rng.standard_normal(A.nnz)
    A.sort_indices()
    b = rng.standard_normal(40)
    b[3] = -0.0
    b[7] = 0.0
    c = rng.standard_normal(m)
    for iters in (1, 2):
        for rhs in (b, None):
            x0 = poly_model.sweep(A, None, rhs, c, iters, x_is_zero=True)
            x1 = poly_model.sweep(A, np.zeros(40), rhs, c, iters)
            assert np.array_equal(x0.view(np.int64), x1.view(np.int64))


def test_chebyshev_coefficients_helper_matches_setup_chebyshev():
    from mlamg.multigrid import chebyshev_coefficients
    rho = 7.25
    c = chebyshev_coefficients(rho, degree=3)
    want = -chebyshev_polynomial_coefficients(rho / 30.0, rho * 1.1, 3)[:-1]
    assert c.shape == (3,) and np.array_equal(c, want)
    c4 = chebyshev_coefficients(rho, 4, 0.1, 1.05)
    assert np.array_equal(c4, -chebyshev_polynomial_coefficients(rho * 0.1, rho * 1.05, 4)[:-1])
