"""Host checks of tests/lsqr_model.py, the model that tests/test_gpu_lsqr.py pins the device LSQR
to. No GPU needed.

* the fast reductions are bitwise the slow transcription of the reduction order;
* the restatement, given scipy's norm and scipy's square, is scipy.sparse.linalg.lsqr bit for bit
  on every case;
* given the device's norm and square it reaches the stop code each case is built for, and the
  cases between them reach 0, 1, 2, 3, 4, 5 and 7. (Code 6 needs 1 + 1/acond <= 1 before tests 4
  and 5 fire; diagonals down to 1e-30 with every tolerance at 0 end on 4 or 5 first.)
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import lsqr_model as lm
from reduce_order import ill_scaled, sum_ref, sumsq_ref, thread_sums, block_totals, partials_total


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def slow_sumsq_512(a):
    return partials_total(block_totals(thread_sums(a * a, 512, 256)), 256)


# ---------------------------------------------------------------- fast reductions
@pytest.mark.parametrize("kind", ("ill_scaled", "minus_zero"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 131072, 131073, 262145))
def test_fast_reductions_are_the_transcription(n, kind):
    x = ill_scaled(n, n) if kind == "ill_scaled" else np.full(n, -0.0)
    assert np.array_equal(bits(lm.sum_512(x)), bits(sum_ref(x)))
    assert np.array_equal(bits(lm.sumsq_512(x)), bits(slow_sumsq_512(x)))
    if kind == "minus_zero":
        assert not np.signbit(lm.sum_512(x))  # every accumulator starts at +0.0
    if n <= 256 * 256:
        # at most 256 partials: mlamg_norm2's grid and 1024-thread finish add the same numbers
        # in the same order, plus zeros
        assert np.array_equal(bits(lm.sumsq_512(x)), bits(sumsq_ref(x)))


def test_empty_vector_sums_to_plus_zero():
    s = lm.sum_512(np.zeros(0))
    assert s == 0.0 and not np.signbit(s)


# ---------------------------------------------------------------- scipy
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_restatement_is_scipy(name):
    """With np.linalg.norm and v**2 the model is scipy's lsqr: x, istop and itn bit for bit."""
    A, b, kw = lm.case(name)
    xs, istop, itn = spla.lsqr(A, b, **kw)[:3]
    x, istop_m, itn_m = lm.lsqr(A, b, norm=np.linalg.norm, square=lm.square_pow, **kw)
    print(f"{name}: scipy istop={istop} itn={itn}")
    assert (istop_m, itn_m) == (istop, itn)
    assert np.array_equal(bits(x), bits(xs))


# ---------------------------------------------------------------- stop codes
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_device_order_model_reaches_the_case_stop_code(name):
    A, b, kw = lm.case(name)
    x, istop, itn = lm.model(name)
    _, want_istop, want_itn = lm.CASES[name]
    print(f"{name}: {A.shape[0]} x {A.shape[1]} {kw} -> istop={istop} itn={itn}")
    assert istop == want_istop
    if want_itn is not None:
        assert itn == want_itn
    assert x.shape == (A.shape[1],) and np.all(np.isfinite(x))
    if want_istop == 0:
        assert not np.any(x) and not np.any(np.signbit(x))


def test_cases_cover_every_reachable_stop_code():
    assert {lm.model(name)[1] for name in lm.CASES} == {0, 1, 2, 3, 4, 5, 7}


def test_one_by_one_takes_the_beta_zero_step():
    """[[2.5]] x = [1]: u = A v - alfa u is exactly 0 on step 1, so beta == 0 and neither anorm
    nor v is updated; the rotation is the identity and x = phi / rho = 1 / 2.5."""
    A, b, kw = lm.case("one_by_one")
    norms = []

    def norm(a):
        norms.append(float(lm.norm_512(a)))
        return lm.norm_512(a)

    x, istop, itn = lm.lsqr(A, b, norm=norm, **kw)
    assert norms[:3] == [1.0, 2.5, 0.0]  # ||b||, ||A^T u||, beta of step 1
    assert (istop, itn) == (1, 1) and x[0] == 1.0 / 2.5


def test_emptied_row_gives_an_exact_zero_gradient():
    A, b, _ = lm.case("b_on_emptied_row")
    assert A[7].nnz == 0 and not np.any(A.T @ b)


# ---------------------------------------------------------------- the singular cycle
@pytest.mark.parametrize("key,smoother", (("n2d", "gauss_seidel"), ("n1d", "jacobi")))
def test_singular_cycle_is_the_oracle_to_lsqr_tolerance(golden_singular, oracle, key, smoother):
    """The model cycle differs from oracle.restated.amg_2_v only in the order of three
    reductions; LSQR at atol = btol = 1e-6 amplifies that, so the two are compared loosely here
    (two cycles). What is asserted bit for bit is the device against the model, on the GPU."""
    from conftest import golden_csr
    g = golden_singular
    A, P = golden_csr(g, f"{key}_A"), golden_csr(g, f"{key}_P")
    b, x0 = g[f"{key}_b"], g[f"{key}_x0"]
    x, err, stops = lm.singular_cycle(A, P, b, x0, smoother=smoother, max_iter=2)
    xo, _, erro, _ = oracle.amg_2_v(A, P, b, x0, error_tol=0.0, max_iter=2, singular=True,
                                    smoother=smoother)
    print(f"{key} {smoother}: coarse solves {stops} err {err} oracle {erro}")
    assert len(err) == len(erro) == 2 and len(stops) == 2
    assert np.allclose(err, erro, rtol=1e-3, atol=0)
    assert np.abs(x - xo).max() <= 1e-3 * np.abs(xo).max()
    if key == "n1d":
        assert stops == [(7, 2 * P.shape[1])] * 2  # every coarse solve ends on iter_lim
