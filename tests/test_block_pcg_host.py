"""CPU: the block PCG entry points (mlamg_pcg_solve_mv, mlamg_pcg_iters_mv) are
exported, bound, and validate their arguments before any device call (no GPU needed: the
pointers below are never dereferenced, every call fails its argument check first)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")


def test_symbols_are_exported_and_bound():
    from mlamg import _lib
    raw = ctypes.CDLL(LIB)
    for name in ("mlamg_pcg_solve_mv", "mlamg_pcg_iters_mv"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def test_arguments_are_checked_without_gpu():
    from mlamg import _lib
    lib = _lib.lib
    solver = ctypes.create_string_buffer(64)  # stands for a solver handle; never read
    b = (ctypes.c_double * 8)()
    x = (ctypes.c_double * 8)()
    it = (ctypes.c_int32 * 64)()
    C, B, X = (ctypes.cast(p, ctypes.c_void_p) for p in (solver, b, x))

    def refused(rc, word):
        assert rc == _lib.MLAMG_EINVAL, (rc, word)
        msg = lib.mlamg_last_error()
        assert b"mlamg_pcg_" in msg and word in msg, msg

    refused(lib.mlamg_pcg_solve_mv(None, B, 4, X, 4, 4, None), b"C is NULL")
    refused(lib.mlamg_pcg_solve_mv(C, None, 4, X, 4, 4, None), b"B is NULL")
    refused(lib.mlamg_pcg_solve_mv(C, B, 4, None, 4, 4, None), b"X is NULL")
    refused(lib.mlamg_pcg_solve_mv(C, B, 4, X, 4, 0, None), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_pcg_solve_mv(C, B, 65, X, 65, 65, None), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_pcg_solve_mv(C, B, 3, X, 4, 4, None), b"ldb < k")
    refused(lib.mlamg_pcg_solve_mv(C, B, 4, X, 3, 4, None), b"ldx < k")
    refused(lib.mlamg_pcg_solve_mv(C, B, 4, B, 4, 4, None), b"B and X must differ")
    refused(lib.mlamg_pcg_iters_mv(None, it, 4, None), b"C is NULL")
    refused(lib.mlamg_pcg_iters_mv(C, None, 4, None), b"iters is NULL")
    refused(lib.mlamg_pcg_iters_mv(C, it, 0, None), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_pcg_iters_mv(C, it, 65, None), b"k must be in [1, MLAMG_MV_MAX")
    with pytest.raises(_lib.MlamgError, match="ldb < k"):
        _lib.call("mlamg_pcg_solve_mv", C, B, 1, X, 4, 2, None)
