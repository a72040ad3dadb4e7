"""CPU: the host side of the batched amg_loss (mlamg.loss.AmgLossBatch): the new
C entries are declared, bound and exported and validate their arguments before any device call;
the stacking helper; every refusal of the batch is raised on the host and names the problem."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mlamg.h")

NEW = ("mlamg_norm2_seg_mv", "mlamg_remove_mean_seg_mv", "mlamg_blockdense_create",
       "mlamg_blockdense_destroy", "mlamg_blockdense_info", "mlamg_blockdense_solve_mv")


@pytest.fixture(scope="module")
def L():
    from mlamg import _lib
    return _lib


@pytest.fixture(scope="module")
def loss():
    import mlamg.loss
    return mlamg.loss


def test_new_symbols_declared_bound_exported(L):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mlamg_[A-Za-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in L.SIGNATURES, name
        assert hasattr(L.lib, name), name
    assert "typedef struct mlamg_blockdense mlamg_blockdense;" in src


def _err(L, rc):
    assert rc == L.MLAMG_EINVAL
    return L.lib.mlamg_last_error().decode()


def test_segmented_entries_validate_before_any_device_call(L):
    x = (ctypes.c_double * 64)()
    off = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    X, O = ctypes.addressof(x), ctypes.addressof(off)
    n2, rm = L.lib.mlamg_norm2_seg_mv, L.lib.mlamg_remove_mean_seg_mv
    for fn, name, tail in ((n2, "mlamg_norm2_seg_mv", (X, None)),
                           (rm, "mlamg_remove_mean_seg_mv", (None,))):
        def call(Xp=X, ld=4, k=4, Op=O, nb=3, ml=1):
            return fn(Xp, ld, k, Op, nb, ml, *tail)
        msg = _err(L, call(Xp=None))
        assert name in msg and "X is NULL" in msg
        msg = _err(L, call(Op=None))
        assert name in msg and "seg_offsets is NULL" in msg
        for k in (0, -1, 65):
            msg = _err(L, call(k=k, ld=65))
            assert name in msg and "k must be in [1, MLAMG_MV_MAX = 64]" in msg
        msg = _err(L, call(ld=3))
        assert name in msg and "ldx < k" in msg
        for nb in (0, -2):
            msg = _err(L, call(nb=nb))
            assert name in msg and "nb must be in" in msg
    msg = _err(L, n2(X, 4, 4, O, 3, 1, None, None))
    assert "mlamg_norm2_seg_mv" in msg and "out is NULL" in msg


def test_blockdense_entries_validate_before_any_device_call(L):
    fake = (ctypes.c_char * 4096)()  # stands for a handle: no check below may read through it
    H = ctypes.addressof(fake)
    off = (ctypes.c_int64 * 2)(0, 0)
    O = ctypes.addressof(off)
    out = ctypes.c_void_p()
    create = L.lib.mlamg_blockdense_create
    msg = _err(L, create(None, O, 1, ctypes.byref(out), None))
    assert "mlamg_blockdense_create" in msg and "A is NULL" in msg
    msg = _err(L, create(H, None, 1, ctypes.byref(out), None))
    assert "mlamg_blockdense_create" in msg and "offsets_host is NULL" in msg
    msg = _err(L, create(H, O, 1, None, None))
    assert "mlamg_blockdense_create" in msg and "out is NULL" in msg
    for nb in (0, -1):
        msg = _err(L, create(H, O, nb, ctypes.byref(out), None))
        assert "mlamg_blockdense_create" in msg and "nb must be in" in msg
    b = (ctypes.c_double * 64)()
    x = (ctypes.c_double * 64)()
    B, X = ctypes.addressof(b), ctypes.addressof(x)
    solve = L.lib.mlamg_blockdense_solve_mv
    for args, what in (((None, B, 4, X, 4, 4), "D is NULL"), ((H, None, 4, X, 4, 4), "B is NULL"),
                       ((H, B, 4, None, 4, 4), "X is NULL"),
                       ((H, B, 4, X, 4, 0), "k must be in [1, MLAMG_MV_MAX = 64]"),
                       ((H, B, 65, X, 65, 65), "k must be in [1, MLAMG_MV_MAX = 64]"),
                       ((H, B, 3, X, 4, 4), "ldb < k"), ((H, B, 4, X, 3, 4), "ldx < k"),
                       ((H, B, 4, B, 4, 4), "B and X must differ")):
        msg = _err(L, solve(*args, None))
        assert "mlamg_blockdense_solve_mv" in msg and what in msg, (args, msg)
    assert _err(L, L.lib.mlamg_blockdense_info(None, None, None, None)).count("D is NULL")
    assert L.lib.mlamg_blockdense_destroy(None) == L.MLAMG_OK


def _blocks(seed=0, sizes=((5, 2), (1, 1), (12, 4), (7, 3))):
    rng = np.random.default_rng(seed)
    As, Ps = [], []
    for n, nc in sizes:
        A = sp.random(n, n, density=0.4, random_state=rng.integers(1 << 30), format="csr")
        A = sp.csr_matrix(A + sp.eye(n))
        A.sort_indices()
        P = sp.random(n, nc, density=0.6, random_state=rng.integers(1 << 30), format="csr")
        P.sort_indices()
        As.append(A)
        Ps.append(P)
    return As, Ps


def test_stacking_offsets_and_segments(loss):
    As, Ps = _blocks()
    st = loss.stack_problems(As, Ps)
    assert st.row_offsets.tolist() == [0, 5, 6, 18, 25]
    assert st.coarse_offsets.tolist() == [0, 2, 3, 7, 10]
    assert st.nnz_offsets.tolist() == np.concatenate([[0], np.cumsum([P.nnz for P in Ps])]).tolist()
    for a in (st.row_offsets, st.coarse_offsets, st.nnz_offsets, st.row_seg, st.entry_seg):
        assert a.dtype == np.int64
    assert st.row_seg.tolist() == [0] * 5 + [1] + [2] * 12 + [3] * 7
    assert st.entry_seg.tolist() == sum(([i] * P.nnz for i, P in enumerate(Ps)), [])
    for i, P in enumerate(Ps):  # the entries of problem i are P_i's, in its stored order
        a, b = st.nnz_offsets[i], st.nnz_offsets[i + 1]
        assert np.array_equal(st.P.data[a:b], P.data)
        assert np.array_equal(st.P.indices[a:b], P.indices + st.coarse_offsets[i])


def test_stack_equals_block_diag_in_canonical_order(loss):
    As, Ps = _blocks(seed=3)
    st = loss.stack_problems(As, Ps)
    for got, mats in ((st.A, As), (st.P, Ps)):
        want = sp.block_diag(mats, format="csr")
        want.sort_indices()
        assert got.shape == want.shape and got.has_canonical_format
        assert got.indptr.dtype == np.int32 and got.indices.dtype == np.int32
        assert np.array_equal(got.indptr, want.indptr)
        assert np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data)


def test_refusals_are_raised_on_the_host_and_name_the_problem(loss, monkeypatch):
    import torch
    import mlamg.sparse

    def no_device():
        raise AssertionError("device work before a refusal")
    monkeypatch.setattr(mlamg.sparse, "_device", no_device)
    As, Ps = _blocks(seed=5)
    B = loss.AmgLossBatch
    with pytest.raises(NotImplementedError, match="neumann_solve_fix"):
        B(As, Ps, 3, neumann_solve_fix=True)
    with pytest.raises(NotImplementedError, match="neumann_solve_fix"):
        loss.amg_loss_and_grad_batch(Ps, As, 3, neumann_solve_fix=True)
    # a P that is not canonical: two column indices of one row of problem 2 swapped
    P = Ps[2]
    idx = P.indices.copy()
    r = int(np.argmax(np.diff(P.indptr) >= 2))
    a = P.indptr[r]
    idx[a], idx[a + 1] = idx[a + 1], idx[a]
    bad = sp.csr_matrix((P.data, idx, P.indptr), shape=P.shape)
    with pytest.raises(ValueError, match=r"problem 2: .*canonical"):
        B(As, Ps[:2] + [bad] + Ps[3:], 3)
    # mismatched shapes
    with pytest.raises(ValueError, match=r"problem 1: P has 5 rows, A has 1"):
        B(As, [Ps[0], Ps[0]] + Ps[2:], 3)
    with pytest.raises(ValueError, match="as many prolongators"):
        B(As, Ps[:3], 3)
    with pytest.raises(ValueError, match=r"problem 3: test_vecs must be \(7, k\)"):
        B(As, Ps, [np.ones((A.shape[0], 2)) for A in As[:3]] + [np.ones((6, 2))])
    with pytest.raises(ValueError, match=r"problem 1: .*k is the same"):
        B(As, Ps, [np.ones((5, 2)), np.ones((1, 3)), np.ones((12, 2)), np.ones((7, 2))])
    # k > 64
    with pytest.raises(ValueError, match="1 to 64"):
        B(As, Ps, 65)
    with pytest.raises(ValueError, match=r"problem 0: .*1 to 64"):
        B(As, Ps, [np.ones((A.shape[0], 65)) for A in As])
    # tot_num_loop < 2 for the gradient
    with pytest.raises(ValueError, match="tot_num_loop"):
        loss.amg_loss_and_grad_batch(Ps, As, 3, tot_num_loop=1)
    # test_vecs / A requiring grad
    Xs = [torch.ones((A.shape[0], 2), dtype=torch.float64) for A in As]
    Xs[2].requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"problem 2\): test_vecs requires grad"):
        B(As, Ps, Xs)
    A1 = As[1].tocoo()
    At = torch.sparse_coo_tensor(np.vstack([A1.row, A1.col]), A1.data, A1.shape,
                                 requires_grad=True)
    with pytest.raises(NotImplementedError, match=r"problem 1\): A requires grad"):
        B([As[0], At] + As[2:], Ps, 3)
    # a coarse block at the method-2 threshold
    thr = loss.batch_coarse_max_rows()
    assert thr == int(os.environ.get("MLAMG_DENSE_TRI_MIN", 2048))
    big_A = sp.eye(2 * thr, format="csr")
    big_P = sp.csr_matrix((np.ones(2 * thr), np.arange(2 * thr) // 2, np.arange(2 * thr + 1)),
                          shape=(2 * thr, thr))
    with pytest.raises(ValueError, match=rf"problem 1: .*{thr} rows.*single call"):
        B([As[0], big_A], [Ps[0], big_P], 3)
    # a stack beyond int32 (the check reads shapes and counts only)
    huge = types.SimpleNamespace(shape=(2**30, 2**30), nnz=7)
    hugeP = types.SimpleNamespace(shape=(2**30, 4), nnz=7)
    with pytest.raises(ValueError, match="row count .*int32"):
        loss.stack_problems([huge] * 2, [hugeP] * 2)
    many = types.SimpleNamespace(shape=(10, 10), nnz=2**30)
    with pytest.raises(ValueError, match="nnz of A .*int32"):
        loss.stack_problems([many] * 2, [types.SimpleNamespace(shape=(10, 4), nnz=7)] * 2)
    with pytest.raises(ValueError, match="nnz of P .*int32"):
        loss.stack_problems([types.SimpleNamespace(shape=(10, 10), nnz=7)] * 2,
                            [types.SimpleNamespace(shape=(10, 4), nnz=2**30)] * 2)
