"""GPU: mlamg_lsqr (csrc/lsqr.hip) and the singular two-level solve built on it, bit for bit
against the host model of tests/lsqr_model.py.

The model is scipy's LSQR with the two things the device does differently substituted: norms in
the fixed order of csrc/reduce.hpp, and squares by multiplication where scipy calls pow
(tests/test_lsqr_model_host.py pins the model to scipy with those two switched back). Everything
else on the path is already scipy's bits (CSR-stream SpMV, residual, restrict, prolong, Galerkin,
transpose, Gauss-Seidel, Jacobi), so x, istop and itn must be the model's exactly, at every stop
code the cases reach: 0, 1, 2, 3, 4, 5 and 7.

Every device call writes into an x that is NaN beforehand and has a 3-entry tail that must come
back untouched, and leaves b as it was. No fallback tolerance is used anywhere in this file.
"""
import ctypes

import numpy as np
import pytest

import lsqr_model as lm

pytestmark = pytest.mark.gpu

TAIL = np.array([1.25, -2.5, 3.75])
EXACT_FORMATS = ("sell", "sorted", "long", "sell_dict", "rowpat")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.multigrid
    import mlamg.sparse
    return mlamg


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def raw_lsqr(ml, torch, Ad, ATd, b, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=None):
    """mlamg_lsqr through the C ABI on a NaN-filled x with a sentinel tail -> (x, istop, itn)."""
    from mlamg._lib import call, ptr, stream_ptr
    n = Ad.shape[1]
    bd = torch.as_tensor(np.array(b, dtype=np.float64)).cuda()
    xd = torch.full((n + len(TAIL),), float("nan"), dtype=torch.float64, device="cuda")
    xd[n:] = torch.as_tensor(TAIL).cuda()
    istop, itn = ctypes.c_int(-1), ctypes.c_int(-1)
    call("mlamg_lsqr", Ad.handle, ATd.handle, ptr(bd), ptr(xd), float(atol), float(btol),
         float(conlim), int(iter_lim or 0), ctypes.byref(istop), ctypes.byref(itn), stream_ptr())
    out = xd.cpu().numpy()
    assert np.array_equal(bits(out[n:]), bits(TAIL)), "wrote past x[n)"
    assert np.array_equal(bits(bd.cpu().numpy()), bits(b)), "b changed"
    return out[:n], int(istop.value), int(itn.value)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_lsqr_is_the_model(ml, torch_cuda, name):
    A, b, kw = lm.case(name)
    xm, istop, itn = lm.model(name)
    _, want_istop, want_itn = lm.CASES[name]
    assert istop == want_istop and (want_itn is None or itn == want_itn)  # the case still bites
    b_in = b.copy()
    x, istop_d, itn_d = ml.multigrid.lsqr(A, b_in, **kw)
    print(f"{name}: model istop={istop} itn={itn}; device istop={istop_d} itn={itn_d} "
          f"max|dx|={np.abs(x - xm).max() if len(xm) else 0.0:.3e}")
    assert (istop_d, itn_d) == (istop, itn)
    assert np.array_equal(bits(x), bits(xm))
    assert np.array_equal(bits(b_in), bits(b))
    Ad =ml.sparse.DeviceCSR.from_scipy(A)
    x, istop_d, itn_d = raw_lsqr(ml, torch_cuda, Ad, Ad.transpose(), b, **kw)
    assert (istop_d, itn_d) == (istop, itn)
    assert np.array_equal(bits(x), bits(xm))
    if istop == 0:
        assert not np.any(x) and not np.any(np.signbit(x))


# ---------------------------------------------------------------- storage formats
def test_exact_formats_give_the_same_bits(ml, torch_cuda):
    """A and its transpose in each format that sums in scipy's order ('vector' has its own)."""
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    A, b, kw = lm.case("neumann_consistent")
    xm, istop, itn = lm.model("neumann_consistent")
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    ATd = Ad.transpose()
    accepted = []
    for fmt in EXACT_FORMATS:
        try:
            Ad.set_format(fmt)
            ATd.set_format(fmt)
        except MlamgError as e:
            assert e.code == MLAMG_EUNSUPPORTED, (fmt, e)
            continue
        assert Ad.get_format()[0] == fmt and ATd.get_format()[0] == fmt
        accepted.append(fmt)
        x, istop_d, itn_d = ml.multigrid.lsqr(Ad, b.copy(), AT=ATd, **kw)
        assert (istop_d, itn_d) == (istop, itn), fmt
        assert np.array_equal(bits(x), bits(xm)), fmt
        x, istop_d, itn_d = raw_lsqr(ml, torch_cuda, Ad, ATd, b, **kw)
        assert (istop_d, itn_d) == (istop, itn), fmt
        assert np.array_equal(bits(x), bits(xm)), fmt
    print(f"exact formats accepted: {accepted}")
    assert {"sell", "sorted"} <= set(accepted)


def test_bad_transpose_is_refused(ml, torch_cuda):
    from mlamg._lib import MLAMG_EINVAL, MlamgError
    A, b, _ = lm.case("tall_consistent")
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    with pytest.raises(MlamgError, match="AT must be A's transpose") as e:
        ml.multigrid.lsqr(Ad, b.copy(), AT=Ad)
    assert e.value.code == MLAMG_EINVAL


# ---------------------------------------------------------------- the singular cycle
def golden_problem(g, key):
    from conftest import golden_csr
    return golden_csr(g, f"{key}_A"), golden_csr(g, f"{key}_P"), g[f"{key}_b"], g[f"{key}_x0"]


@pytest.mark.parametrize("smoother", ("gauss_seidel", "jacobi"))
@pytest.mark.parametrize("key,max_iter", (("n2d", 6), ("n1d", 4)))
def test_singular_cycle_error_history_is_the_model(golden_singular, ml, oracle, key, max_iter,
                                                   smoother):
    """amg_2_v(singular=True, error_tol=...): the iterate and the whole ||x|| history, bit for
    bit. On n1d every coarse solve runs into iter_lim = 2 n_c (istop 7 after 200 iterations)."""
    A, P, b, x0 = golden_problem(golden_singular, key)
    xm, errm, stops = lm.singular_cycle(A, P, b, x0, smoother=smoother, tol=1e-9,
                                        max_iter=max_iter)
    x, conv, err, it = ml.multigrid.amg_2_v(A, P, b, x0, singular=True, error_tol=1e-9,
                                            max_iter=max_iter, smoother=smoother)
    print(f"{key} {smoother}: coarse solves {stops}\n  model  {errm}\n  device {err}")
    if key == "n1d":
        assert stops == [(7, 2 * P.shape[1])] * max_iter
    assert it == len(err) == len(errm) == max_iter
    assert np.array_equal(bits(err), bits(errm))
    assert np.array_equal(bits(x), bits(xm))


@pytest.mark.parametrize("smoother", ("gauss_seidel", "jacobi"))
def test_singular_cycle_residual_history(golden_singular, ml, oracle, smoother):
    """The same with res_tol on n1d: the final iterate bit for bit (it passes through every
    cycle's LSQR), the history within 1e-13 of np.linalg.norm(b - A @ x_i) of the model's
    iterates (the fused residual norm has a format-dependent order; the bound is
    test_spmv_residual_bitwise's)."""
    A, P, b, x0 = golden_problem(golden_singular, "n1d")
    xm, errm, stops = lm.singular_cycle(A, P, b, x0, smoother=smoother, tol=1e-8,
                                        res_tol_mode=True, max_iter=4)
    x, conv, err, it = ml.multigrid.amg_2_v(A, P, b, x0, singular=True, res_tol=1e-8,
                                            max_iter=4, smoother=smoother)
    print(f"n1d {smoother} res_tol: coarse solves {stops}\n  model  {errm}\n  device {err}")
    assert it == len(err) == len(errm) == 4
    assert np.array_equal(bits(x), bits(xm))
    assert np.all(np.abs(err - errm) <= 1e-13 * errm)
