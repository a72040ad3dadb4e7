"""CPU: the block Gauss-Seidel entry points (mlamg_gs_sweep_mv, mlamg_gs_mv_path,
mlamg_hier_set_mv_gauss_seidel) are exported, bound, and validate their arguments
before any device call (no GPU needed: the pointers below are never dereferenced, every call
fails its argument check first)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")

NAMES = ("mlamg_gs_sweep_mv", "mlamg_gs_mv_path", "mlamg_gs_path",
         "mlamg_hier_set_mv_gauss_seidel")


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
    b = (ctypes.c_double * 8)()
    x = (ctypes.c_double * 8)()
    path = ctypes.c_int32(-7)
    G, B, X = (ctypes.cast(p, ctypes.c_void_p) for p in (handle, b, x))

    def refused(rc, word):
        assert rc == _lib.MLAMG_EINVAL, (rc, word)
        msg = lib.mlamg_last_error()
        assert b"mlamg_" in msg and word in msg, msg

    refused(lib.mlamg_gs_sweep_mv(None, X, 4, B, 4, 4, 1, None), b"G is NULL")
    refused(lib.mlamg_gs_sweep_mv(G, None, 4, B, 4, 4, 1, None), b"X is NULL")
    refused(lib.mlamg_gs_sweep_mv(G, X, 4, B, 4, 0, 1, None), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_gs_sweep_mv(G, X, 65, B, 65, 65, 1, None), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_gs_sweep_mv(G, X, 3, B, 4, 4, 1, None), b"ldx < k")
    refused(lib.mlamg_gs_sweep_mv(G, X, 4, B, 3, 4, 1, None), b"ldb < k")
    refused(lib.mlamg_gs_sweep_mv(G, X, 4, X, 4, 4, 1, None), b"B and X must differ")
    refused(lib.mlamg_gs_mv_path(None, 4, ctypes.byref(path)), b"G is NULL")
    refused(lib.mlamg_gs_mv_path(G, 4, None), b"path is NULL")
    refused(lib.mlamg_gs_mv_path(G, 0, ctypes.byref(path)), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_gs_mv_path(G, 65, ctypes.byref(path)), b"k must be in [1, MLAMG_MV_MAX")
    refused(lib.mlamg_gs_path(None, 0, ctypes.byref(path)), b"G is NULL")
    refused(lib.mlamg_gs_path(G, 0, None), b"path is NULL")
    refused(lib.mlamg_gs_path(G, -1, ctypes.byref(path)), b"which must be 0")
    refused(lib.mlamg_gs_path(G, 2, ctypes.byref(path)), b"which must be 0")
    assert path.value == -7
    refused(lib.mlamg_hier_set_mv_gauss_seidel(None, 1), b"H is NULL")
    with pytest.raises(_lib.MlamgError, match="G is NULL"):
        _lib.call("mlamg_gs_sweep_mv", None, X, 4, B, 4, 4, 1, None)
