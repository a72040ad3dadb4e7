"""CPU: the multi-vector (n x k) C-ABI is declared, bound and validates its arguments before any
device call; the amg_loss formula (ns/model/loss.py:92-94) on a hand-made history."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

MV_NAMES = ("mlamg_spmm", "mlamg_residual_mv", "mlamg_jacobi_mv", "mlamg_restrict_mv",
            "mlamg_prolong_add_mv", "mlamg_norm2_mv", "mlamg_remove_mean_mv",
            "mlamg_dense_solve_mv", "mlamg_hier_vcycle_mv")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")


def test_header_declares_multivector_entries():
    src = open(os.path.join(ROOT, "include", "mlamg.h")).read()
    for name in MV_NAMES:
        assert f"int {name}(" in src, name
    assert "#define MLAMG_MV_MAX 64" in src


@needs_lib
def test_multivector_entries_bound_and_exported():
    from mlamg import _lib
    for name in MV_NAMES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name


@needs_lib
def test_spmm_validates_before_any_device_call():
    from mlamg import _lib
    lib = _lib.lib
    rc = lib.mlamg_spmm(None, None, 8, None, 8, 8, 1.0, 0.0, None)
    assert rc == _lib.MLAMG_EINVAL
    assert b"NULL" in lib.mlamg_last_error()
    # non-NULL arguments that are never dereferenced: k and ld are checked first
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for k, ldx, ldy, word in ((0, 8, 8, b"k must be"), (65, 80, 80, b"k must be"),
                              (8, 7, 8, b"leading dimension"), (8, 8, 7, b"leading dimension")):
        rc = lib.mlamg_spmm(p, p, ldx, p, ldy, k, 1.0, 0.0, None)
        assert rc == _lib.MLAMG_EINVAL, (k, ldx, ldy)
        assert word in lib.mlamg_last_error(), (k, ldx, ldy, lib.mlamg_last_error())


@needs_lib
def test_other_entries_validate_before_any_device_call():
    from mlamg import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    calls = {
        "mlamg_residual_mv": lambda k, ld: (p, p, ld, p, ld, p, ld, k, None, None),
        "mlamg_jacobi_mv": lambda k, ld: (p, p, p, ld, p, ld, p, ld, k, 1, None),
        "mlamg_restrict_mv": lambda k, ld: (p, p, ld, p, ld, k, None),
        "mlamg_prolong_add_mv": lambda k, ld: (p, p, ld, p, ld, k, None),
        "mlamg_norm2_mv": lambda k, ld: (p, ld, 1, k, p, None),
        "mlamg_remove_mean_mv": lambda k, ld: (p, ld, 1, k, None),
        "mlamg_dense_solve_mv": lambda k, ld: (p, p, ld, p, ld, k, None),
        "mlamg_hier_vcycle_mv": lambda k, ld: (p, p, ld, p, ld, k, 1, 0, 0, None, None),
    }
    for name, args in calls.items():
        f = getattr(lib, name)
        for k, ld in ((0, 8), (65, 80), (8, 7)):
            assert f(*args(k, ld)) == _lib.MLAMG_EINVAL, (name, k, ld)
            assert lib.mlamg_last_error(), name
    assert lib.mlamg_hier_vcycle_mv(None, None, 8, None, 8, 8, 1, 0, 0, None, None) \
        == _lib.MLAMG_EINVAL
    assert b"NULL" in lib.mlamg_last_error()
    with pytest.raises(_lib.MlamgError):
        _lib.call("mlamg_norm2_mv", None, 8, 4, 8, None, None)


@needs_lib
def test_loss_formula_matches_numpy():
    from mlamg.loss import loss_from_errs
    import mlamg
    assert mlamg.loss.loss_from_errs is loss_from_errs
    errs = np.array([[1.0, 2.0, 0.5, 3.0],
                     [0.5, 1.5, 0.4, 1.0],
                     [0.3, 1.0, 0.3, 0.5],
                     [0.2, 0.9, 0.25, 0.1],
                     [0.1, 0.5, 0.2, 0.02]])
    loss, convs = loss_from_errs(errs)
    want_convs = (errs[-1] / errs[-3]) ** (1 / 2)
    e = np.exp(want_convs)
    want_loss = (e / e.sum()) @ want_convs
    assert np.allclose(convs, want_convs, rtol=1e-15, atol=0)
    # the exported function shifts by max(convs) before exp: a few roundings apart (exp, the
    # normalisation, a 4-term dot product: well under 50 ulp)
    assert abs(loss - want_loss) <= 50 * np.finfo(np.float64).eps * abs(want_loss)
    with pytest.raises(ValueError):
        loss_from_errs(errs[:2])


@needs_lib
def test_amg_loss_refuses_neumann_fix():
    import scipy.sparse as sp
    from mlamg.loss import amg_loss
    A = sp.eye(4, format="csr")
    with pytest.raises(NotImplementedError):
        amg_loss(A, A, 2, neumann_solve_fix=True)
