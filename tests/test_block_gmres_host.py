"""CPU: the block GMRES entry point (mlamg_gmres_mv) is exported, bound, and
validates its arguments before any device call (no GPU needed: the pointers below are never
dereferenced, every call fails its argument check first)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")


def test_symbol_is_exported_and_bound():
    from mlamg import _lib
    raw = ctypes.CDLL(LIB)
    assert hasattr(raw, "mlamg_gmres_mv")
    assert "mlamg_gmres_mv" in _lib.SIGNATURES


def test_python_surface_exists():
    from mlamg.hierarchy import Hierarchy
    assert callable(getattr(Hierarchy, "gmres_multi"))


def test_arguments_are_checked_without_gpu():
    from mlamg import _lib
    lib = _lib.lib
    mat = ctypes.create_string_buffer(64)    # stands for a matrix handle; never read
    hier = ctypes.create_string_buffer(64)   # ... a hierarchy handle
    b = (ctypes.c_double * 8)()
    x = (ctypes.c_double * 8)()
    info = (ctypes.c_int32 * 64)()
    it = (ctypes.c_int32 * 64)()
    A, M, B, X = (ctypes.cast(p, ctypes.c_void_p) for p in (mat, hier, b, x))

    def solve(A=A, M=M, B=B, ldb=4, X=X, ldx=4, k=4, info=info, it=it):
        return lib.mlamg_gmres_mv(A, M, B, ldb, X, ldx, k, 1e-8, 5, 10, 1, info, it, None, 0, None)

    def refused(rc, word):
        assert rc == _lib.MLAMG_EINVAL, (rc, word)
        msg = lib.mlamg_last_error()
        assert b"mlamg_gmres_mv" in msg and word in msg, msg

    refused(solve(A=None), b"A is NULL")
    refused(solve(M=None), b"M is NULL")
    refused(solve(B=None), b"B is NULL")
    refused(solve(X=None), b"X is NULL")
    refused(solve(info=None), b"info is NULL")
    refused(solve(it=None), b"inner_iters is NULL")
    refused(solve(k=0), b"k must be in [1, MLAMG_MV_MAX")
    refused(solve(k=65, ldb=65, ldx=65), b"k must be in [1, MLAMG_MV_MAX")
    refused(solve(ldb=3), b"ldb < k")
    refused(solve(ldx=3), b"ldx < k")
    refused(solve(X=B), b"B and X must differ")
    with pytest.raises(_lib.MlamgError, match="ldb < k"):
        _lib.call("mlamg_gmres_mv", A, M, B, 1, X, 4, 2, 1e-8, 5, 10, 1, info, it, None, 0, None)
