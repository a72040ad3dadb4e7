"""GPU: the multi-vector kernels in the canonical CSR-vector order (mlamg_spmm_vec and its kin,
DeviceCSR.matmat(order=...)) and the block V-cycle on VECTOR-format operators
(Hierarchy.enable_block_vector); DESIGN.md §22.

The acceptance criterion is §17's with the VECTOR format active: column j of every block result is
bitwise the single-vector result on column j, and the plain product is bitwise oracle.c
vec_matvec. Every comparison is np.array_equal; test_the_two_orders_differ shows that a kernel
summing in scipy's order could not pass."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 9, 16, 17, 64)
WIDTHS = (64, 128, 256, 512)
HEAD = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1537, 2049, 4100)
# name: (seed, rows, columns, maxlen)
SHAPES = {"a": (8, 160, 6000, 1500), "b": (9, 96, 70000, 1500), "c": (10, 1200, 1200, 1200)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.hierarchy
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


def _call(name, *args):
    from mlamg._lib import call
    return call(name, *args)


def _ragged(seed, n_rows, n_cols, maxlen):
    """Distinct sorted columns per row; the first rows have the lengths of HEAD that fit the
    shape (row-length edges of the 64-lane waves and the 512-entry stripes), the rest are
    uniform in [0, maxlen)."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(0, maxlen, n_rows)
    head = [m for m in HEAD if m <= n_cols]
    lens[:len(head)] = head
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rs.choice(n_cols, m, replace=False)) for m in lens])
    data = rs.randn(indptr[-1]) - 0.1
    A = sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)),
                      shape=(n_rows, n_cols))
    assert A.has_sorted_indices and np.array_equal(np.diff(A.indptr), lens)
    return A


@pytest.fixture(scope="module")
def cases(oracle):
    """Per matrix: A, a 64-column operand block and oracle.vec_matvec of each of its columns
    (computed once; the tests take the leading k columns)."""
    out = {}
    for name, (seed, n_rows, n_cols, maxlen) in SHAPES.items():
        A = _ragged(seed, n_rows, n_cols, maxlen)
        X = np.random.RandomState(seed + 100).standard_normal((n_cols, 64))
        ref = np.stack([oracle.vec_matvec(A, X[:, j]) for j in range(64)], axis=1)
        out[name] = (A, X, ref)
    return out


def test_the_two_orders_differ(cases):
    """The canonical order and scipy's give different bits in at least half of the rows with
    three or more entries, in every column: these inputs tell the two orders apart."""
    for name, (A, X, ref) in cases.items():
        rows = np.diff(A.indptr) >= 3
        for j in range(9):
            differ = int(np.count_nonzero((ref[:, j] != A @ X[:, j]) & rows))
            assert 2 * differ >= int(rows.sum()), (name, j, differ, int(rows.sum()))
        assert np.allclose(ref, A @ X, rtol=1e-10, atol=1e-10)


def _spmm_vec(torch, Ad, X, k, alpha=1.0, beta=0.0, Y=None):
    from mlamg._lib import ptr, stream_ptr
    if Y is None:
        Y = torch.full((Ad.shape[0], k), np.nan, dtype=torch.float64, device="cuda")
    _call("mlamg_spmm_vec", Ad.handle, ptr(X), X.stride(0), ptr(Y), Y.stride(0), k, alpha, beta,
          stream_ptr())
    return Y


@pytest.mark.parametrize("name,idx16", (("a", True), ("a", False), ("b", False)))
def test_spmm_vec_is_the_canonical_order(ml, torch_cuda, cases, monkeypatch, name, idx16):
    """mlamg_spmm_vec into a NaN-filled Y is oracle.vec_matvec per column and matvec per column
    with the VECTOR format active; the block does not depend on the active width or format.
    (a): 16-bit column copies, and 32-bit indices under MLAMG_NO_IDX16; (b): 70,000 columns."""
    torch = torch_cuda
    A, Xh, ref = cases[name]
    if name == "a" and not idx16:
        monkeypatch.setenv("MLAMG_NO_IDX16", "1")
    assert (A.shape[1] <= 65536) == (name == "a")
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    for i, k in enumerate(KS):
        X = dev(torch, Xh[:, :k])
        blocks = []
        for w in WIDTHS:
            Ad.set_format("vector", w)
            assert Ad.get_format()[:2] == ("vector", w)
            blocks.append(host(_spmm_vec(torch, Ad, X, k)))
            if w == WIDTHS[i % 4]:
                for j in range(k):
                    yj = host(Ad.matvec(X[:, j].contiguous()))
                    assert np.array_equal(blocks[-1][:, j], yj), (k, w, j)
        Ad.set_format("csr_stream")
        blocks.append(host(_spmm_vec(torch, Ad, X, k)))
        assert np.array_equal(blocks[0], ref[:, :k]), k
        for Y in blocks[1:]:
            assert np.array_equal(Y, blocks[0]), k


def test_alpha_beta_slices_and_argument_checks(ml, torch_cuda, cases):
    torch = torch_cuda
    from mlamg._lib import MLAMG_EINVAL, MlamgError, ptr, stream_ptr
    A, Xh, ref = cases["a"]
    n_rows, n_cols = A.shape
    Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("vector", 256)
    k = 9
    X = dev(torch, Xh[:, :k])
    Y0 = dev(torch, np.random.RandomState(3).standard_normal((n_rows, k)))
    for alpha, beta in ((-1.0, 1.0), (0.5, 2.0)):
        Y = _spmm_vec(torch, Ad, X, k, alpha, beta, Y0.clone())
        for j in range(k):
            yj = Y0[:, j].contiguous()
            Ad.matvec(X[:, j].contiguous(), out=yj, alpha=alpha, beta=beta)
            assert np.array_equal(host(Y[:, j]), host(yj)), (alpha, beta, j)
    # column slices of wider tensors: (offset 1, odd ld) takes the 8-byte instantiation,
    # (offset 2, even ld) on 16-byte aligned storage the 16-byte one
    sentinel = -123.5
    for k in (5, 8):
        e = 1 - (k & 1)
        for off, width in ((1, k + 2 + e), (2, k + 3 + e)):
            assert (width & 1) == (off & 1)
            xb = torch.full((n_cols, width), 7.25, dtype=torch.float64, device="cuda")
            xb[:, off:off + k] = dev(torch, Xh[:, :k])
            yb = torch.full((n_rows, width), sentinel, dtype=torch.float64, device="cuda")
            Xs, Ys = xb[:, off:off + k], yb[:, off:off + k]
            assert (Xs.data_ptr() % 16 == 0) == (off == 2) and Xs.stride(0) == width
            _spmm_vec(torch, Ad, Xs, k, Y=Ys)
            o = host(yb)
            assert np.array_equal(o[:, off:off + k], ref[:, :k]), (k, off)
            assert np.all(np.delete(o, np.s_[off:off + k], axis=1) == sentinel), (k, off)
            assert np.all(np.delete(host(xb), np.s_[off:off + k], axis=1) == 7.25)
    # k and the leading dimensions
    Y = torch.empty((n_rows, 65), dtype=torch.float64, device="cuda")
    X65 = torch.ones((n_cols, 65), dtype=torch.float64, device="cuda")
    with pytest.raises(MlamgError, match="k must be in") as ei:
        _call("mlamg_spmm_vec", Ad.handle, ptr(X65), 65, ptr(Y), 65, 65, 1.0, 0.0, stream_ptr())
    assert ei.value.code == MLAMG_EINVAL
    with pytest.raises(MlamgError, match="ldx < k"):
        _call("mlamg_spmm_vec", Ad.handle, ptr(X65), 7, ptr(Y), 65, 8, 1.0, 0.0, stream_ptr())
    with pytest.raises(MlamgError, match="ldy < k"):
        _call("mlamg_spmm_vec", Ad.handle, ptr(X65), 65, ptr(Y), 7, 8, 1.0, 0.0, stream_ptr())
    with pytest.raises(ValueError):
        Ad.matmat(X65, order="vector")


def test_epilogues_match_the_single_entries(ml, torch_cuda, cases):
    """On the square matrix (c), VECTOR format active: residual (with B and B = NULL) and its
    norms, Jacobi at nu = 1 and 3, prolongation add — per column the single entries' bits."""
    torch = torch_cuda
    from mlamg._lib import ptr, stream_ptr
    A, Xh, _ = cases["c"]
    n = A.shape[0]
    k = 6
    Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("vector", 128)
    rs = np.random.RandomState(2)
    X = dev(torch, Xh[:, :k])
    B = dev(torch, rs.standard_normal((n, k)))
    s = stream_ptr()
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    for Bm in (B, None):
        R = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
        norms = torch.empty(k, dtype=torch.float64, device="cuda")
        _call("mlamg_residual_mv_vec", Ad.handle, ptr(Bm), k, ptr(X), k, ptr(R), k, k, ptr(norms),
              s)
        for j in range(k):
            r = torch.empty(n, dtype=torch.float64, device="cuda")
            bj = B[:, j].contiguous() if Bm is not None else zero
            _call("mlamg_residual", Ad.handle, ptr(bj), ptr(X[:, j].contiguous()), ptr(r), None, s)
            assert np.array_equal(host(R[:, j]), host(r)), j
            nj = torch.empty(1, dtype=torch.float64, device="cuda")
            _call("mlamg_norm2", ptr(r), n, ptr(nj), s)
            assert host(norms)[j] == host(nj)[0], j
    dinv = dev(torch, 0.5 / (1.0 + np.abs(rs.standard_normal(n))))
    for nu in (1, 3):
        Xm = X.clone()
        T = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
        _call("mlamg_jacobi_mv_vec", Ad.handle, ptr(dinv), ptr(B), k, ptr(Xm), k, ptr(T), k, k, nu,
              s)
        for j in range(k):
            xj = X[:, j].contiguous()
            tj = torch.empty_like(xj)
            _call("mlamg_jacobi", Ad.handle, ptr(dinv), ptr(B[:, j].contiguous()), ptr(xj),
                  ptr(tj), nu, s)
            assert np.array_equal(host(Xm[:, j]), host(xj)), (nu, j)
    E = X
    X0 = dev(torch, rs.standard_normal((n, k)))
    Xa = X0.clone()
    _call("mlamg_prolong_add_mv_vec", Ad.handle, ptr(E), k, ptr(Xa), k, k, s)
    for j in range(k):
        xj = X0[:, j].contiguous()
        _call("mlamg_prolong_add", Ad.handle, ptr(E[:, j].contiguous()), ptr(xj), s)
        assert np.array_equal(host(Xa[:, j]), host(xj)), j


def test_matmat_order(ml, torch_cuda, cases):
    torch = torch_cuda
    A, Xh, ref = cases["a"]
    k = 9
    X = dev(torch, Xh[:, :k])
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    today = host(Ad.matmat(X))
    assert np.array_equal(today, A @ Xh[:, :k])
    assert np.array_equal(host(Ad.matmat(X, order="csr")), today)
    assert np.array_equal(host(Ad.matmat(X, order="vector")), ref[:, :k])
    for fmt in (("csr_stream", 0), ("vector", 64), ("vector", 512)):
        Ad.set_format(*fmt)
        Y = host(Ad.matmat(X, order="active"))
        assert np.array_equal(Y, ref[:, :k] if fmt[0] == "vector" else today), fmt
        for j in range(k):
            assert np.array_equal(Y[:, j], host(Ad.matvec(X[:, j].contiguous()))), (fmt, j)
        assert np.array_equal(host(Ad @ X), today)  # A @ X stays matmat(X)
    Y0 = dev(torch, np.random.RandomState(4).standard_normal((A.shape[0], k)))
    out = Y0.clone()
    assert Ad.matmat(X, out=out, alpha=0.5, beta=2.0, order="vector").data_ptr() == out.data_ptr()
    yj = Y0[:, 0].contiguous()
    Ad.matvec(X[:, 0].contiguous(), out=yj, alpha=0.5, beta=2.0)
    assert np.array_equal(host(out[:, 0]), host(yj))
    with pytest.raises(ValueError, match="order"):
        Ad.matmat(X, order="scipy")


# ---------------------------------------------------------------- the block cycle
def _single_loop(torch, H, b, x, n_cycles, norm, remove_mean):
    """n_cycles single-vector cycles on (b, x), each followed by the mean removal (if asked)
    and mlamg_norm2 of the freshly computed residual (or of x): the history cycle_multi is
    defined by."""
    from mlamg._lib import ptr, stream_ptr
    A = H.levels[0].A
    n = x.numel()
    s = stream_ptr()
    bz = b if b is not None else torch.zeros(n, dtype=torch.float64, device="cuda")
    hist = []
    for _ in range(n_cycles):
        H.cycle(bz, x, 1, use_graph=False, history=False)
        if remove_mean:
            _call("mlamg_remove_mean", ptr(x), n, s)
        v = x
        if norm == "residual":
            v = torch.empty(n, dtype=torch.float64, device="cuda")
            _call("mlamg_residual", A.handle, ptr(bz), ptr(x), ptr(v), None, s)
        nj = torch.empty(1, dtype=torch.float64, device="cuda")
        _call("mlamg_norm2", ptr(v), n, ptr(nj), s)
        hist.append(host(nj)[0])
    return np.array(hist)


def _forced(ml, first_level):
    """The 48 x 48 Poisson hierarchy with A, P and R of every level >= first_level forced into
    the VECTOR format, the widths cycling through 64 / 128 / 256 / 512."""
    H = ml.hierarchy.Hierarchy.build(ml.problems.poisson_2d_5pt(48), max_coarse=100,
                                     fine_format="csr_stream", coarse_format="exact")
    assert H.n_levels >= 3
    i = 0
    for L in H.levels[first_level:]:
        for M in (L.A, L.P, L.R):
            M.set_format("vector", WIDTHS[i % 4])
            assert M.get_format()[:2] == ("vector", WIDTHS[i % 4])
            i += 1
    for L in H.levels[:first_level]:
        assert all(M.get_format()[0] != "vector" for M in (L.A, L.P, L.R))
    return H


@pytest.fixture(scope="module")
def forced(ml):
    return {1: _forced(ml, 1), 0: _forced(ml, 0)}


@pytest.mark.parametrize("nu", ((1, 1), (2, 1), (0, 1)))
@pytest.mark.parametrize("first_level", (1, 0))
def test_block_cycle_on_vector_operators(ml, torch_cuda, forced, first_level, nu):
    """first_level 1: the coarse levels' operators in the VECTOR format, level 0 in scipy's
    order (formats mix within the cycle); 0: level 0's too, where the caller's leading
    dimension reaches the canonical-order kernel."""
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    H = forced[first_level]
    n = H.levels[0].A.shape[0]
    k, cycles = 6, 4
    rs = np.random.RandomState(7)
    X0 = dev(torch, rs.standard_normal((n, k)))
    B = dev(torch, rs.standard_normal((n, k)))
    refusal = r"an operator is in the VECTOR format, whose row order is not scipy's"
    with pytest.raises(MlamgError, match=refusal) as ei:
        H.cycle_multi(B, X0.clone(), 1)
    assert ei.value.code == MLAMG_EUNSUPPORTED
    assert H.enable_block_vector() is H
    _call("mlamg_hier_set_smoothing", H.handle, nu[0], nu[1])
    try:
        for norm, remove_mean, Bm in (("residual", False, B), ("x", True, B),
                                      ("residual", True, None), ("x", False, None)):
            X = X0.clone()
            hist = H.cycle_multi(Bm, X, cycles, norm=norm, remove_mean=remove_mean)
            assert hist.shape == (cycles, k)
            X2 = X0.clone()
            hist2 = H.cycle_multi(Bm, X2, cycles, norm=norm, remove_mean=remove_mean)
            assert np.array_equal(host(X), host(X2)) and np.array_equal(hist, hist2)
            for j in range(k):
                xj = X0[:, j].contiguous()
                bj = Bm[:, j].contiguous() if Bm is not None else None
                hj = _single_loop(torch, H, bj, xj, cycles, norm, remove_mean)
                assert np.array_equal(host(X[:, j]), host(xj)), (norm, remove_mean, j)
                assert np.array_equal(hist[:, j], hj), (norm, remove_mean, j, hist[:, j], hj)
        # a column slice of a wider iterate, history off
        wide = torch.full((n, k + 1), 3.0, dtype=torch.float64, device="cuda")
        wide[:, :k] = X0
        assert H.cycle_multi(B, wide[:, :k], cycles, history=False) is None
        Xc = X0.clone()
        H.cycle_multi(B, Xc, cycles, history=False)
        assert np.array_equal(host(wide)[:, :k], host(Xc)) and np.all(host(wide)[:, k] == 3.0)
        if nu == (1, 1):
            Z = H.precondition(B)
            for j in range(k):
                zj = H.precondition(B[:, j].contiguous())
                assert np.array_equal(host(Z[:, j]), host(zj)), j
        # the switch off again: the refusal, word for word
        H.enable_block_vector(False)
        with pytest.raises(MlamgError, match=refusal) as ei:
            H.cycle_multi(B, X0.clone(), 1)
        assert ei.value.code == MLAMG_EUNSUPPORTED
    finally:
        H.enable_block_vector(False)
        _call("mlamg_hier_set_smoothing", H.handle, 1, 1)


def test_composes_with_block_gauss_seidel(ml, torch_cuda):
    """pyamg_sa (symmetric Gauss-Seidel on every level) with level 1's A in the VECTOR format:
    both switches on, the block cycle is the single cycles."""
    torch = torch_cuda
    from mlamg._lib import MlamgError
    H = ml.hierarchy.Hierarchy.pyamg_sa(ml.problems.poisson_2d_5pt(48))
    assert H.n_levels >= 3
    H.levels[1].A.set_format("vector", 128)
    n, k, cycles = H.levels[0].A.shape[0], 5, 3
    rs = np.random.RandomState(9)
    B = dev(torch, rs.standard_normal((n, k)))
    X0 = dev(torch, rs.standard_normal((n, k)))
    H.enable_block_gauss_seidel()
    with pytest.raises(MlamgError, match="VECTOR"):
        H.cycle_multi(B, X0.clone(), 1)
    H.enable_block_vector()
    X = X0.clone()
    hist = H.cycle_multi(B, X, cycles)
    for j in range(k):
        xj = X0[:, j].contiguous()
        hj = _single_loop(torch, H, B[:, j].contiguous(), xj, cycles, "residual", False)
        assert np.array_equal(host(X[:, j]), host(xj)), j
        assert np.array_equal(hist[:, j], hj), j
