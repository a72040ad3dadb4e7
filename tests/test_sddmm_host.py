"""CPU: mlamg_sddmm (the sampled dense-dense product, include/mlamg.h) is declared, bound and
validates its arguments before any device call, naming the argument at fault; the gradient
surface of mlamg.loss refuses what it does not differentiate without touching a device."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")


def test_header_declares_sddmm():
    src = open(os.path.join(ROOT, "include", "mlamg.h")).read()
    assert "int mlamg_sddmm(" in src
    assert "SUMMATION ORDER" in src


@needs_lib
def test_sddmm_bound_and_exported():
    from mlamg import _lib
    assert "mlamg_sddmm" in _lib.SIGNATURES
    assert hasattr(_lib.lib, "mlamg_sddmm")
    assert len(_lib.SIGNATURES["mlamg_sddmm"][1]) == 10


@needs_lib
def test_sddmm_validates_before_any_device_call():
    from mlamg import _lib
    lib = _lib.lib
    # non-NULL arguments that are never dereferenced: every check comes before the handle is read
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for args, word in (((None, p, 8, p, 8, 8, 1.0, 0.0, p, None), b"S is NULL"),
                       ((p, None, 8, p, 8, 8, 1.0, 0.0, p, None), b"U is NULL"),
                       ((p, p, 8, None, 8, 8, 1.0, 0.0, p, None), b"V is NULL"),
                       ((p, p, 8, p, 8, 8, 1.0, 0.0, None, None), b"out is NULL"),
                       ((p, p, 8, p, 8, 0, 1.0, 0.0, p, None), b"k must be"),
                       ((p, p, 80, p, 80, 65, 1.0, 0.0, p, None), b"k must be"),
                       ((p, p, 7, p, 8, 8, 1.0, 0.0, p, None), b"ldu < k"),
                       ((p, p, 8, p, 7, 8, 1.0, 0.0, p, None), b"ldv < k")):
        assert lib.mlamg_sddmm(*args) == _lib.MLAMG_EINVAL, word
        msg = lib.mlamg_last_error()
        assert word in msg and b"mlamg_sddmm" in msg, (word, msg)
    with pytest.raises(_lib.MlamgError, match="S is NULL"):
        _lib.call("mlamg_sddmm", None, None, 8, None, 8, 8, 1.0, 0.0, None, None)


@needs_lib
def test_gradient_surface_is_exported_and_refuses_on_the_host():
    import scipy.sparse as sp
    import torch
    import mlamg.loss as ml
    for name in ("amg_loss", "amg_loss_and_grad", "amg_loss_values", "loss_from_errs"):
        assert name in ml.__all__ and callable(getattr(ml, name)), name
    A = sp.eye(4, format="csr")
    with pytest.raises(NotImplementedError, match="neumann_solve_fix"):
        ml.amg_loss_and_grad(A, A, 2, neumann_solve_fix=True)
    x = torch.ones((4, 2), dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="test_vecs"):
        ml.amg_loss_and_grad(A, A, x)
    # unsorted column indices: refused before anything is uploaded
    P = sp.csr_matrix((np.ones(3), np.array([1, 0, 1]), np.array([0, 2, 3, 3, 3])), shape=(4, 2))
    with pytest.raises(ValueError, match="canonical"):
        ml.amg_loss_and_grad(P, A, 2)
    v = torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="canonical"):
        ml.amg_loss_values(v, P.indptr, P.indices, P.shape, A, 2)
    with pytest.raises(NotImplementedError, match="test_vecs"):
        ml.amg_loss_values(v, np.array([0, 1, 2, 3, 3]), np.array([0, 1, 0]), (4, 2), A, x)
    with pytest.raises(TypeError):
        ml.amg_loss_values(v.float(), np.array([0, 1, 2, 3, 3]), np.array([0, 1, 0]), (4, 2), A, 2)
