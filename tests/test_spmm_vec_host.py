"""CPU: the canonical-order multi-vector entry points (mlamg_spmm_vec, mlamg_residual_mv_vec,
mlamg_jacobi_mv_vec, mlamg_prolong_add_mv_vec, mlamg_hier_set_mv_vector) are
exported, bound, and validate their arguments before any device call (no GPU needed: the pointers
below are never dereferenced, every call fails its argument check first)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")

NAMES = ("mlamg_spmm_vec", "mlamg_residual_mv_vec", "mlamg_jacobi_mv_vec",
         "mlamg_prolong_add_mv_vec", "mlamg_hier_set_mv_vector")
K_MSG = b"k must be in [1, MLAMG_MV_MAX"


def test_symbols_are_exported_and_bound():
    from mlamg import _lib
    raw = ctypes.CDLL(LIB)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def test_arguments_are_checked_without_gpu():
    from mlamg import _lib
    lib = _lib.lib
    handle = ctypes.create_string_buffer(64)  # stands for a handle; never read
    bufs = [(ctypes.c_double * 8)() for _ in range(4)]
    A = ctypes.cast(handle, ctypes.c_void_p)
    X, Y, B, D = (ctypes.cast(p, ctypes.c_void_p) for p in bufs)

    def refused(rc, word):
        assert rc == _lib.MLAMG_EINVAL, (rc, word)
        msg = lib.mlamg_last_error()
        assert b"mlamg_" in msg and word in msg, msg

    # mlamg_spmm_vec(A, X, ldx, Y, ldy, k, alpha, beta, stream)
    refused(lib.mlamg_spmm_vec(None, X, 4, Y, 4, 4, 1.0, 0.0, None), b"A is NULL")
    refused(lib.mlamg_spmm_vec(A, None, 4, Y, 4, 4, 1.0, 0.0, None), b"X is NULL")
    refused(lib.mlamg_spmm_vec(A, X, 4, None, 4, 4, 1.0, 0.0, None), b"Y is NULL")
    refused(lib.mlamg_spmm_vec(A, X, 4, Y, 4, 0, 1.0, 0.0, None), K_MSG)
    refused(lib.mlamg_spmm_vec(A, X, 65, Y, 65, 65, 1.0, 0.0, None), K_MSG)
    refused(lib.mlamg_spmm_vec(A, X, 3, Y, 4, 4, 1.0, 0.0, None), b"ldx < k")
    refused(lib.mlamg_spmm_vec(A, X, 4, Y, 3, 4, 1.0, 0.0, None), b"ldy < k")
    refused(lib.mlamg_spmm_vec(A, X, 4, X, 4, 4, 1.0, 0.0, None), b"X and Y must differ")
    # mlamg_residual_mv_vec(A, B, ldb, X, ldx, R, ldr, k, norms, stream)
    refused(lib.mlamg_residual_mv_vec(None, B, 4, X, 4, Y, 4, 4, None, None), b"A is NULL")
    refused(lib.mlamg_residual_mv_vec(A, B, 4, None, 4, Y, 4, 4, None, None), b"X is NULL")
    refused(lib.mlamg_residual_mv_vec(A, B, 4, X, 4, None, 4, 4, None, None), b"R is NULL")
    refused(lib.mlamg_residual_mv_vec(A, B, 4, X, 4, Y, 4, 0, None, None), K_MSG)
    refused(lib.mlamg_residual_mv_vec(A, B, 65, X, 65, Y, 65, 65, None, None), K_MSG)
    refused(lib.mlamg_residual_mv_vec(A, B, 4, X, 3, Y, 4, 4, None, None), b"ldx < k")
    refused(lib.mlamg_residual_mv_vec(A, B, 4, X, 4, Y, 3, 4, None, None), b"ldr < k")
    refused(lib.mlamg_residual_mv_vec(A, B, 3, X, 4, Y, 4, 4, None, None), b"ldb < k")
    refused(lib.mlamg_residual_mv_vec(A, None, 0, X, 4, X, 4, 4, None, None),
            b"X and R must differ")
    # mlamg_jacobi_mv_vec(A, dinv_w, B, ldb, X, ldx, X_tmp, ldt, k, nu, stream)
    refused(lib.mlamg_jacobi_mv_vec(None, D, B, 4, X, 4, Y, 4, 4, 1, None), b"A is NULL")
    refused(lib.mlamg_jacobi_mv_vec(A, None, B, 4, X, 4, Y, 4, 4, 1, None), b"dinv_w is NULL")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, None, 4, Y, 4, 4, 1, None), b"X is NULL")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, X, 4, None, 4, 4, 1, None), b"X_tmp is NULL")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, X, 4, Y, 4, 0, 1, None), K_MSG)
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 65, X, 65, Y, 65, 65, 1, None), K_MSG)
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, X, 3, Y, 4, 4, 1, None), b"ldx < k")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, X, 4, Y, 3, 4, 1, None), b"ldt < k")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 3, X, 4, Y, 4, 4, 1, None), b"ldb < k")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, X, 4, Y, 4, 4, -1, None), b"nu < 0")
    refused(lib.mlamg_jacobi_mv_vec(A, D, B, 4, X, 4, X, 4, 4, 1, None),
            b"X_tmp must differ from X")
    # mlamg_prolong_add_mv_vec(P, E, lde, X, ldx, k, stream)
    refused(lib.mlamg_prolong_add_mv_vec(None, B, 4, X, 4, 4, None), b"P is NULL")
    refused(lib.mlamg_prolong_add_mv_vec(A, None, 4, X, 4, 4, None), b"E is NULL")
    refused(lib.mlamg_prolong_add_mv_vec(A, B, 4, None, 4, 4, None), b"X is NULL")
    refused(lib.mlamg_prolong_add_mv_vec(A, B, 4, X, 4, 0, None), K_MSG)
    refused(lib.mlamg_prolong_add_mv_vec(A, B, 65, X, 65, 65, None), K_MSG)
    refused(lib.mlamg_prolong_add_mv_vec(A, B, 3, X, 4, 4, None), b"lde < k")
    refused(lib.mlamg_prolong_add_mv_vec(A, B, 4, X, 3, 4, None), b"ldx < k")
    refused(lib.mlamg_hier_set_mv_vector(None, 1), b"H is NULL")
    with pytest.raises(_lib.MlamgError, match="A is NULL") as ei:
        _lib.call("mlamg_spmm_vec", None, X, 4, Y, 4, 4, 1.0, 0.0, None)
    assert ei.value.code == _lib.MLAMG_EINVAL


def test_matmat_order_is_checked_first():
    """An unknown order raises before the handle or the tensors are looked at (no device)."""
    from mlamg.sparse import DeviceCSR
    A = object.__new__(DeviceCSR)  # no handle: nothing below may reach the library
    with pytest.raises(ValueError, match="order"):
        A.matmat(None, order="bogus")
