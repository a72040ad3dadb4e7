"""GPU parity of the storage formats and of the multilevel hierarchy (setup + V-cycle executor)
against the oracle, plus full-size (C4) properties."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_csr

pytestmark = pytest.mark.gpu

MATS = ("c1", "p2d", "lap3d", "rnd")


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


def dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


@pytest.mark.parametrize("k", MATS)
@pytest.mark.parametrize("fmt", ("sell", "csr_stream", "auto_exact", "sorted", "sell_dict",
                                 "rowpat", "long"))
def test_exact_formats_bitwise(golden, ml, torch_cuda, k, fmt):
    torch = torch_cuda
    A = golden_csr(golden, k)
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    try:
        Ad.set_format(fmt)
    except MlamgError as e:  # sell_dict / rowpat on operators with many distinct values
        assert fmt in ("sell_dict", "rowpat") and e.code == MLAMG_EUNSUPPORTED
        assert Ad.get_format()[0] == "csr_stream"
    x = dev(torch, golden[f"{k}_x"])
    assert np.array_equal(Ad.matvec(x).cpu().numpy(), golden[f"{k}_Ax"])
    from mlamg._lib import call, ptr, stream_ptr
    b = dev(torch, golden[f"{k}_b"])
    r = torch.empty_like(b)
    nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
    call("mlamg_residual", Ad.handle, ptr(b), ptr(x), ptr(r), ptr(nrm), stream_ptr())
    assert np.array_equal(r.cpu().numpy(), golden[f"{k}_resid"])
    ref = np.linalg.norm(golden[f"{k}_resid"])
    assert abs(nrm.item() - ref) <= 1e-13 * ref


@pytest.mark.parametrize("n_cols,idx16", [(700, True), (700, False), (65536, True),
                                          (70000, False)])
def test_vector_format_one_order_for_every_width(ml, oracle, torch_cuda, monkeypatch, n_cols,
                                                 idx16):
    """CSR-vector widths 64..512 compute one canonical order (oracle.c vec_matvec), for every
    epilogue; rows from empty to several 512-entry stripes; other widths are refused. With
    16-bit column copies (n_cols <= 65536) and with the 32-bit indices (env MLAMG_NO_IDX16,
    or more than 65536 columns: the last column 65535 / 69999 is always referenced)."""
    torch = torch_cuda
    from mlamg._lib import MlamgError, call, ptr, stream_ptr
    if not idx16:
        monkeypatch.setenv("MLAMG_NO_IDX16", "1")
    rs = np.random.RandomState(8)
    n = 700
    lens = rs.randint(0, 1500, n)
    lens[::13] = 0
    lens[5] = 4100
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([rs.randint(0, n_cols, l) for l in lens]).astype(np.int32)
    indices[-1] = n_cols - 1
    A = sp.csr_matrix((rs.randn(indptr[-1]) - 0.1, indices, indptr), shape=(n, n_cols))
    A.sum_duplicates()
    A = (A + sp.diags(np.abs(rs.randn(n)) + 1.0) @ sp.eye(n, n_cols)).tocsr()
    A.sort_indices()
    assert A.indices.max() == n_cols - 1
    x, b, e = rs.randn(n_cols), rs.randn(n), rs.randn(n)
    ref = oracle.vec_matvec(A, x)
    assert np.allclose(ref, A @ x, rtol=1e-11, atol=1e-11)
    # every kernel of the family: k_vcan_wave with x in LDS (MLAMG_VCAN_WAVE=1, n_cols <= 16384)
    # and from global memory (=2), k_csr_vcan at each width (=0, the default)
    for mode, vw in [(m, w) for m in ("1", "2", "0") for w in (0, 64, 128, 256, 512)]:
        monkeypatch.setenv("MLAMG_VCAN_WAVE", mode)
        Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("vector", vw)
        assert Ad.get_format()[0] == "vector"
        xd, bd = dev(torch, x), dev(torch, b)
        assert np.array_equal(Ad.matvec(xd).cpu().numpy(), ref)
        if n_cols == n:  # the residual epilogue needs a square operator
            r = torch.empty_like(bd)
            nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
            call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
            assert np.array_equal(r.cpu().numpy(), b - ref)
            if vw:
                nrm_ref = nrm.item() if (mode, vw) == ("1", 64) else nrm_ref
                assert nrm.item() == nrm_ref  # per-row partials: the norm is width-independent
        y = dev(torch, e)
        call("mlamg_prolong_add", Ad.handle, ptr(xd), ptr(y), stream_ptr())
        assert np.array_equal(y.cpu().numpy(), e + ref)
    for bad in (4, 8, 32, 1024):
        with pytest.raises(MlamgError):
            ml.sparse.DeviceCSR.from_scipy(A).set_format("vector", bad)


def test_long_format_ragged_chunked_and_epilogues(ml, torch_cuda):
    """long format (csrc/spmv.hip k_csr_long): bitwise scipy on ragged rows — empty rows, rows
    of exactly one tile (4096), rows longer than a tile (streamed in chunks), tiles capped at 64
    rows — for y = A x, the residual (+ norm partials), x += A e and the Jacobi sweep."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    rs = np.random.RandomState(11)
    n = 6000
    lens = rs.randint(0, 900, n)
    lens[::41] = 0
    lens[7] = 4096
    lens[8] = 4097
    lens[100] = 5999
    lens[200:330] = rs.randint(0, 5, 130)  # short rows: tiles hit the 64-row cap
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([rs.choice(n, l, replace=False) for l in lens])  # unsorted rows
    A = sp.csr_matrix((rs.randn(indptr[-1]), indices, indptr), shape=(n, n))
    A.setdiag(np.abs(rs.randn(n)) + 1.0)
    A = A.tocsr()
    Ad = ml.sparse.DeviceCSR.from_scipy(A, check=False).set_format("long")
    assert Ad.get_format()[0] == "long"
    A = Ad.to_scipy()  # the stored order the kernel sums in
    x, b, e = rs.randn(n), rs.randn(n), rs.randn(n)
    xd, bd = dev(torch, x), dev(torch, b)
    ref_y = ml.sparse.DeviceCSR.from_scipy(A, check=False)  # csr_stream: scipy's order
    assert np.array_equal(Ad.matvec(xd).cpu().numpy(), A @ x)
    assert np.array_equal(ref_y.matvec(xd).cpu().numpy(), A @ x)
    r = torch.empty_like(bd)
    nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
    call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
    assert np.array_equal(r.cpu().numpy(), b - A @ x)
    assert abs(nrm.item() - np.linalg.norm(b - A @ x)) <= 1e-13 * np.linalg.norm(b - A @ x)
    y = dev(torch, e)
    call("mlamg_prolong_add", Ad.handle, ptr(xd), ptr(y), stream_ptr())
    assert np.array_equal(y.cpu().numpy(), e + A @ x)
    dw = Ad.diag_inv(2.0 / 3.0)
    xs, t = dev(torch, x), torch.empty_like(xd)
    call("mlamg_jacobi", Ad.handle, ptr(dw), ptr(bd), ptr(xs), ptr(t), 1, stream_ptr())
    d = dw.cpu().numpy()
    assert np.array_equal(xs.cpu().numpy(), x + d * (b - A @ x))


def test_results_do_not_depend_on_format_choice(ml, oracle, torch_cuda):
    """the autotune picks among kernels that compute the same bits — the
    exact-order family (scipy's order) for rows shorter than Hierarchy.VEC_MIN_MEAN_ROW, the
    CSR-vector family (one canonical order for every width) for longer coarse rows — so forcing
    any other member of the family on every operator leaves the V-cycle iterate bitwise
    unchanged (the residual norm's partial sums are grouped per kernel block, so the history
    agrees to rounding). The iterate's history matches the oracle cycle, which needs no
    per-operator order information beyond the family."""
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(40)
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    b = np.random.RandomState(1).randn(n)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=300, coarse_format="auto")
    assert H.n_levels >= 3
    ops = [M for L in H.levels for M in (L.A, L.P, L.R)]
    family = ["vector" if M.get_format()[0] == "vector" else "exact" for M in ops]
    outs = []
    exact_forced = ("csr_stream", "long", "sorted", "sell")
    for step in range(5):
        if step > 0:
            for M, fam in zip(ops, family):
                if fam == "vector":
                    M.set_format("vector", (64, 128, 256, 512)[step - 1])
                else:
                    try:
                        M.set_format(exact_forced[step - 1])
                    except ml._lib.MlamgError:
                        M.set_format("csr_stream")
            H.attach_dinvs()
        xd = dev(torch, x0)
        h = H.cycle(dev(torch, b), xd, 4)
        outs.append((xd.cpu().numpy(), h))
    for xo, ho in outs[1:]:
        assert np.array_equal(xo, outs[0][0])
        assert np.allclose(ho, outs[0][1], rtol=1e-13, atol=0)
    lv = _oracle_levels_from_device(H)
    xr, hr = oracle.vcycle_solve(lv, H.Ac.to_scipy(), b, x0, 4)
    assert np.allclose(outs[0][1], hr, rtol=1e-10, atol=0)


def test_vector_family_rule_c3_like(ml, torch_cuda):
    """The family is a rule on the matrix (mean row length), not a timing: two builds choose
    the same family for every operator and give bitwise-identical iterates."""
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(48)
    n = A.shape[0]
    x0 = np.random.RandomState(2).randn(n)
    res = []
    for _ in range(2):
        H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=300)
        fams = [[f[k][0] == "vector" for k in "APR"] for f in H.formats()]
        for L, fam in zip(H.levels, fams):
            for k, M in zip("APR", (L.A, L.P, L.R)):
                long_rows = M.nnz >= H.VEC_MIN_MEAN_ROW * M.shape[0]
                assert fam["APR".index(k)] == (long_rows and L is not H.levels[0])
        xd = dev(torch, x0)
        H.cycle(torch.zeros(n, dtype=torch.float64, device="cuda"), xd, 3)
        res.append((fams, xd.cpu().numpy()))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])


def test_sell_ragged_rows(ml, torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(3)
    n = 1000
    lens = rs.randint(0, 40, n)
    lens[::97] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rs.choice(n, l, replace=False)) for l in lens])
    A = sp.csr_matrix((rs.randn(indptr[-1]), indices, indptr), shape=(n, n))
    x = rs.randn(n)
    for sigma in (1, 128, 512):
        Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("sell", sigma)
        assert Ad.get_format()[:2] == ("sell", sigma)
        assert np.array_equal(Ad.matvec(dev(torch, x)).cpu().numpy(), A @ x)
        from mlamg._lib import call, ptr, stream_ptr
        b = dev(torch, rs.randn(n))
        r = torch.empty_like(b)
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        xd = dev(torch, x)
        call("mlamg_residual", Ad.handle, ptr(b), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
        ref = b.cpu().numpy() - A @ x
        assert np.array_equal(r.cpu().numpy(), ref)
        assert abs(nrm.item() - np.linalg.norm(ref)) <= 1e-13 * np.linalg.norm(ref)


def test_sorted_format_ragged_and_limits(ml, torch_cuda):
    """sorted format: bitwise CSR order on ragged rows (empty rows, rows spanning several
    blocks' worth of columns), and EUNSUPPORTED (format unchanged) past its limits."""
    torch = torch_cuda
    from mlamg._lib import MlamgError, call, ptr, stream_ptr
    rs = np.random.RandomState(5)
    n, m = 3000, 200000
    lens = rs.randint(0, 300, n)
    lens[::37] = 0
    lens[5] = 4096  # exactly one full block
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rs.choice(m, l, replace=False)) for l in lens])
    A = sp.csr_matrix((rs.randn(indptr[-1]), indices, indptr), shape=(n, m))
    x = rs.randn(m)
    Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("sorted")
    assert Ad.get_format()[0] == "sorted"
    assert np.array_equal(Ad.matvec(dev(torch, x)).cpu().numpy(), A @ x)
    Sq = (sp.random(n, n, density=0.01, random_state=rs, format="csr")
          + sp.eye(n, format="csr")).tocsr()
    Sq.sort_indices()
    Sd = ml.sparse.DeviceCSR.from_scipy(Sq).set_format("sorted")
    xs, b = rs.randn(n), rs.randn(n)
    r = torch.empty(n, dtype=torch.float64, device="cuda")
    nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
    bd, xd = dev(torch, b), dev(torch, xs)  # keep the device copies alive across the call
    call("mlamg_residual", Sd.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
    ref = b - Sq @ xs
    assert np.array_equal(r.cpu().numpy(), ref)
    assert abs(nrm.item() - np.linalg.norm(ref)) <= 1e-13 * np.linalg.norm(ref)
    # a row longer than one block
    L = sp.csr_matrix((np.ones(5000), np.arange(5000), [0, 5000]), shape=(1, 5000))
    Ld = ml.sparse.DeviceCSR.from_scipy(L).set_format("sell")
    with pytest.raises(MlamgError):
        Ld.set_format("sorted")
    assert Ld.get_format()[0] == "sell"
    # a block whose columns need two windows (owned | far ghosts) is supported ...
    mw = (1 << 21) + 11
    xw = rs.randn(mw)
    W = sp.csr_matrix((rs.randn(4), [0, 7, 1 << 20, (1 << 20) + 3], [0, 2, 4]), shape=(2, mw))
    Wd = ml.sparse.DeviceCSR.from_scipy(W).set_format("sorted")
    assert np.array_equal(Wd.matvec(dev(torch, xw)).cpu().numpy(), W @ xw)
    # ... three far-apart clusters are not
    W3 = sp.csr_matrix((np.ones(3), [0, (1 << 20) + 5, (1 << 21) + 10], [0, 3]), shape=(1, mw))
    W3d = ml.sparse.DeviceCSR.from_scipy(W3)
    with pytest.raises(MlamgError):
        W3d.set_format("sorted")
    assert W3d.get_format()[0] == "csr_stream"
    assert np.array_equal(W3d.matvec(dev(torch, xw)).cpu().numpy(), W3 @ xw)


def test_sorted_value_dictionary(ml, torch_cuda):
    """sorted format with <= 256 distinct values codes them in one byte (SA prolongator of a
    constant-coefficient stencil: 10 values); products and order unchanged."""
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(16)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream")
    P = H.levels[0].P.to_scipy()
    assert len(np.unique(P.data)) <= 256
    Pd = ml.sparse.DeviceCSR.from_scipy(P).set_format("sorted")
    assert Pd.get_format()[:2] == ("sorted", 1)
    rs = np.random.RandomState(3)
    e = rs.randn(P.shape[1])
    ed = dev(torch, e)
    assert np.array_equal(Pd.matvec(ed).cpu().numpy(), P @ e)
    R = P.T.tocsr()
    R.sort_indices()
    Rd = ml.sparse.DeviceCSR.from_scipy(R).set_format("sorted")
    assert Rd.get_format()[:2] == ("sorted", 1)
    r = rs.randn(R.shape[1])
    assert np.array_equal(Rd.matvec(dev(torch, r)).cpu().numpy(), R @ r)
    # many distinct values: plain fp64 values
    Q = sp.random(400, 300, density=0.05, random_state=rs, format="csr")
    Qd = ml.sparse.DeviceCSR.from_scipy(Q).set_format("sorted")
    assert Qd.get_format()[:2] == ("sorted", 0)
    q = rs.randn(300)
    assert np.array_equal(Qd.matvec(dev(torch, q)).cpu().numpy(), Q @ q)


def test_sorted_value_codes(ml, torch_cuda):
    """sorted format with per-block value dictionaries (set_format('sorted', 2): two-byte codes
    into each 4,096-entry block's own list of distinct values): a Galerkin A_1 of a constant
    stencil (few distinct values per block) and a skewed operator (85 % of the entries from 300
    values, the rest ~600 k distinct) — every epilogue bitwise the fp64 form (scipy's order);
    refused (EUNSUPPORTED) where more than half of a block's entries are distinct or a
    one-byte dictionary applies."""
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError, call, ptr, stream_ptr
    rs = np.random.RandomState(12)
    A = ml.problems.poisson_3d_7pt(40)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, fine_format="csr_stream",
                                     finalize=False)
    A1 = H.levels[1].A.to_scipy()
    assert 256 < len(np.unique(A1.data)) < 61440
    # skewed: 85 % of the entries from 300 values, the rest (~80k) all distinct
    n = 40000
    Q = sp.random(n, n, density=2.5e-3, random_state=rs, format="csr") + sp.eye(n, format="csr")
    Q = Q.tocsr()
    Q.sort_indices()
    common = rs.randn(300)
    pick = rs.rand(Q.nnz) < 0.85
    Q.data[pick] = common[rs.randint(0, 300, pick.sum())]
    Q.data[~pick] = rs.randn((~pick).sum())
    assert len(np.unique(Q.data)) > 61440
    for M in (A1, Q):
        Md = ml.sparse.DeviceCSR.from_scipy(M).set_format("sorted", 2)
        assert Md.get_format()[:2] == ("sorted", 2)
        Mf = ml.sparse.DeviceCSR.from_scipy(M).set_format("sorted", 0)
        assert Md.format_bytes() < Mf.format_bytes()
        m = M.shape[0]
        x, b, e = rs.randn(m), rs.randn(m), rs.randn(m)
        xd, bd = dev(torch, x), dev(torch, b)
        assert np.array_equal(Md.matvec(xd).cpu().numpy(), M @ x)
        r = torch.empty_like(bd)
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        call("mlamg_residual", Md.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
        assert np.array_equal(r.cpu().numpy(), b - M @ x)
        y = dev(torch, e)
        call("mlamg_prolong_add", Md.handle, ptr(xd), ptr(y), stream_ptr())
        assert np.array_equal(y.cpu().numpy(), e + M @ x)
    # all values distinct: refused
    W = sp.random(3000, 3000, density=0.02, random_state=rs, format="csr")
    with pytest.raises(MlamgError) as ex:
        ml.sparse.DeviceCSR.from_scipy(W).set_format("sorted", 2)
    assert ex.value.code == MLAMG_EUNSUPPORTED
    # <= 256 values: the one-byte dictionary, as format 'sorted'
    P = H.levels[0].P.to_scipy()
    with pytest.raises(MlamgError):
        ml.sparse.DeviceCSR.from_scipy(P).set_format("sorted", 2)
    # in a hierarchy: the autotune may pick it; the cycle is the fp64 format's bit for bit
    H2 = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, fine_format="csr_stream",
                                      coarse_format="exact")
    x0 = rs.randn(A.shape[0])
    b0 = rs.randn(A.shape[0])
    x1 = dev(torch, x0)
    h1 = H2.cycle(dev(torch, b0), x1, 3)
    H2.levels[1].A.set_format("sorted", 2)
    x2 = dev(torch, x0)
    h2 = H2.cycle(dev(torch, b0), x2, 3)
    assert np.array_equal(h1, h2) and torch.equal(x1, x2)


def test_graph_recaptured_after_format_change(ml, torch_cuda):
    """A captured cycle graph bakes in kernels and format arrays: changing an operator's format
    must force a re-capture (format epoch), and the iterate stays bitwise the same."""
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(20)
    n = A.shape[0]
    rs = np.random.RandomState(4)
    x0, b = rs.randn(n), rs.randn(n)
    bd = dev(torch, b)
    # exact-order formats only, so every storage gives the same bits
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, coarse_format="exact")
    ref = dev(torch, x0)
    h_ref = H.cycle(bd, ref, 4, use_graph=False)
    for fmt in ("csr_stream", "sell_dict", "sorted", "sell", "rowpat"):
        x = dev(torch, x0)
        H.cycle(bd, x, 1, use_graph=True)   # capture with the current formats
        for L in H.levels:                  # then swap every operator's storage
            for M in (L.A, L.P, L.R):
                try:
                    M.set_format(fmt)
                except Exception:
                    M.set_format("csr_stream")
        x = dev(torch, x0)
        h = H.cycle(bd, x, 4, use_graph=True)
        assert torch.equal(x, ref), fmt
        assert np.allclose(h, h_ref, rtol=1e-14, atol=0)


def test_graph_rekeyed_by_every_argument(ml, torch_cuda):
    """A captured cycle bakes in b, x, the history buffer and the tolerance: a call that differs
    in any one of them must re-capture, and a call with the first arguments must not replay a
    later capture. The buffers are held here (Hierarchy.cycle would hand the library a fresh
    history tensor per call), so each step changes exactly one key field. Every iterate is
    bitwise the eager run of the same call, every history equal to it."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    A = ml.problems.poisson_3d_7pt(20)
    n = A.shape[0]
    rs = np.random.RandomState(11)
    x0 = dev(torch, rs.randn(n))
    b1, b2 = dev(torch, rs.randn(n)), dev(torch, rs.randn(n))
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, coarse_format="exact")
    nc = 6

    def run(b, x, hist, tol, use_graph):
        x.copy_(x0)
        if hist is not None:
            hist.zero_()
        done = ctypes.c_int32()
        call("mlamg_hier_vcycle", H.handle, ptr(b), ptr(x), nc, -1.0 if tol is None else tol,
             ptr(hist), ctypes.byref(done), int(use_graph), stream_ptr())
        return x.clone(), None if hist is None else hist[: done.value].cpu().numpy()

    xa, xb, xe = (torch.empty_like(x0) for _ in range(3))
    ha, he = (torch.zeros(nc, dtype=torch.float64, device="cuda") for _ in range(2))
    tol = float(run(b2, xe, he, None, False)[1][2])  # stops the b2 run after its third cycle
    first = (b1, xa, ha, None)
    steps = [first,
             (b2, xa, ha, None),     # another b
             (b2, xb, ha, None),     # another x
             (b2, xb, None, None),   # no history
             (b2, xb, ha, tol),      # a tolerance
             (None, xb, ha, tol),    # a zero right-hand side
             first]
    for i, (b, x, hist, t) in enumerate(steps):
        x_ref, h_ref = run(b, xe, None if hist is None else he, t, False)
        x_got, h_got = run(b, x, hist, t, True)
        assert torch.equal(x_got, x_ref), i
        if hist is not None:
            assert np.array_equal(h_got, h_ref), i
    assert len(run(b2, xb, ha, tol, True)[1]) == 3


def test_sell_dict_format(ml, torch_cuda):
    """Dictionary-coded SELL: bitwise CSR order on a stencil (ragged boundary rows, sigma
    orders), every epilogue through the hierarchy, and refusal past 255 offsets / 256 values."""
    torch = torch_cuda
    from mlamg._lib import MlamgError, call, ptr, stream_ptr
    A = ml.problems.poisson_3d_7pt(20)
    n = A.shape[0]
    rs = np.random.RandomState(7)
    x, b = rs.randn(n), rs.randn(n)
    xd, bd = dev(torch, x), dev(torch, b)
    for sigma in (1, 512):
        Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("sell_dict", sigma)
        assert Ad.get_format()[:2] == ("sell_dict", sigma)
        assert np.array_equal(Ad.matvec(xd).cpu().numpy(), A @ x)
        r = torch.empty(n, dtype=torch.float64, device="cuda")
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
        assert np.array_equal(r.cpu().numpy(), b - A @ x)
    # 2 distinct values incl. a negative zero kept apart from +0
    B = A.copy()
    B.data = B.data.copy()
    B.data[5] = -0.0
    Bd = ml.sparse.DeviceCSR.from_scipy(B).set_format("sell_dict")
    assert np.array_equal(Bd.matvec(xd).cpu().numpy(), B @ x)
    # too many distinct values -> refused, back to CSR-stream, still bitwise
    R = sp.random(500, 500, density=0.05, random_state=rs, format="csr")
    Rd = ml.sparse.DeviceCSR.from_scipy(R)
    with pytest.raises(MlamgError):
        Rd.set_format("sell_dict")
    assert Rd.get_format()[0] == "csr_stream"
    xr = rs.randn(500)
    assert np.array_equal(Rd.matvec(dev(torch, xr)).cpu().numpy(), R @ xr)
    # whole cycle with the fine operator dictionary-coded
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream")
    H2 = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream")
    H2.levels[0].A.set_format("sell_dict")
    x1, x2 = dev(torch, x), dev(torch, x)
    h1 = H.cycle(bd, x1, 5)
    h2 = H2.cycle(bd, x2, 5)
    assert torch.equal(x1, x2)
    assert np.allclose(h1, h2, rtol=1e-14, atol=0)


def _oracle_levels_from_device(H):
    levels = []
    for L in H.levels:
        f = {k: v for k, v in zip("APR", (L.A.get_format(), L.P.get_format(), L.R.get_format()))}
        vw = {k: (v[1] if v[0] == "vector" else 0) for k, v in f.items()}
        levels.append({
            "A": L.A.to_scipy(), "P": L.P.to_scipy(), "R": L.R.to_scipy(),
            "Dw": sp.diags(L.dinv.cpu().numpy()),
            "A_vw": vw["A"], "P_vw": vw["P"], "R_vw": vw["R"],
        })
    return levels


@pytest.mark.parametrize("coarse_format", ("vector", "exact"))
def test_multilevel_setup_and_cycle(ml, oracle, torch_cuda, coarse_format):
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(24)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, coarse_format=coarse_format)
    assert H.n_levels >= 3
    # setup parity: the oracle's recipe with the device's omegas reproduces every level bitwise
    levels, Ac = oracle.build_hierarchy(A, alpha=0.1, max_coarse=100,
                                        omegas=[L.omega for L in H.levels])
    assert len(levels) == len(H.levels)
    for Lo, Ld in zip(levels, H.levels):
        Pd = Ld.P.to_scipy()
        assert np.array_equal(Pd.indptr, Lo["P"].indptr)
        assert np.array_equal(Pd.indices, Lo["P"].indices)  # scipy csr_matmat column order
        assert np.array_equal(Pd.data, Lo["P"].data)
        Ad = Ld.A.to_scipy()
        assert np.array_equal(Ad.indptr, Lo["A"].indptr) and np.array_equal(Ad.data, Lo["A"].data)
        assert np.array_equal(Ld.seeds, Lo["seeds"])
    Acd = H.Ac.to_scipy()
    assert np.array_equal(Acd.indices, Ac.indices) and np.array_equal(Acd.data, Ac.data)
    # lambda_max: Lanczos vs ARPACK on every level
    for Lo, Ld in zip(levels, H.levels):
        ref = oracle.arpack_lambda_max(Lo["A"])
        assert abs(Ld.lam - ref) <= 1e-12 * ref
    # cycle parity: device executor vs the oracle cycle on the device's operators
    lv = _oracle_levels_from_device(H)
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    b = np.random.RandomState(1).randn(n)
    xo, ho = oracle.vcycle_solve(lv, H.Ac.to_scipy(), b, x0, 6)
    for use_graph in (False, True):
        xd = dev(torch, x0)
        hd = H.cycle(dev(torch, b), xd, 6, use_graph=use_graph)
        # everything but the coarsest solve (dense inverse vs SuperLU) is bitwise: the
        # remaining differences are O(1e-16) relative per cycle
        assert np.allclose(hd, ho, rtol=1e-11, atol=0)
        assert np.allclose(xd.cpu().numpy(), xo, rtol=1e-10, atol=1e-12 * np.abs(xo).max())


def test_multilevel_tolerance_stop(ml, torch_cuda):
    torch = torch_cuda
    A = ml.problems.poisson_2d_5pt(64)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=200)
    n = A.shape[0]
    b = dev(torch, np.random.RandomState(2).randn(n))
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    hist = H.cycle(b, x, 200, tol=1e-8)
    assert hist[-1] <= 1e-8 and (len(hist) == 1 or hist[-2] > 1e-8)
    assert np.all(np.diff(np.log(hist)) < 0)
    r = b.cpu().numpy() - A @ x.cpu().numpy()
    assert abs(np.linalg.norm(r) - hist[-1]) <= 1e-12 + 1e-10 * hist[-1]


@pytest.mark.slow
def test_c4_full_size_properties(ml, oracle, torch_cuda):
    """C4 (216^3): fine-level SpMV bitwise vs the C oracle at full size; lambda_max vs the
    analytic value 1 + cos(pi/217); V-cycle residuals decrease monotonically."""
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(216)
    Ad = ml.sparse.DeviceCSR.from_scipy(A, check=False).set_format("auto_exact")
    x = np.random.RandomState(0).randn(A.shape[0])
    y = Ad.matvec(dev(torch, x)).cpu().numpy()
    assert np.array_equal(y, oracle.csr_matvec(A, x))
    lam, its = ml.multigrid.lambda_max_dinv_a(Ad)
    exact = 1.0 + np.cos(np.pi / 217)
    assert abs(lam - exact) <= 1e-12 * exact, (lam, exact, its)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=2000)
    n = A.shape[0]
    xv = dev(torch, x / np.linalg.norm(x))
    hist = H.cycle(torch.zeros(n, dtype=torch.float64, device="cuda"), xv, 12)
    assert np.all(np.diff(hist) < 0)
    conv = (hist[-1] / hist[-4]) ** (1 / 3)
    assert 0.3 < conv < 0.8


@pytest.mark.slow
def test_c4_full_size_hierarchy_parity(ml, oracle, torch_cuda):
    """C4 (216^3, the bench configuration, aggregation='reference' as bench.py) at full size: the
    device hierarchy vs the oracle's build_hierarchy given the device's omegas — every level's seeds, P and A, and the coarsest
    matrix bitwise (the SpGEMM / SA / Bellman-Ford kernels reproduce scipy's results at 70 M
    nonzeros) — then 4 V-cycles of the device executor vs the oracle's cycle on the ORACLE's
    operators (each operator summed in the device kernel's order: scipy order for every exact
    format, the CSR-vector order where the autotune picked it): residual histories within
    rtol 1e-11 (the only non-bitwise step is the coarsest solve, dense inverse vs SuperLU) and
    the iterate within 1e-10 of its max. Reference: ns/lib/multigrid.py:102-108,165;
    MLAMG.py:189-195 per level."""
    import gc
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(216)
    # the bench's aggregation (bench.py defaults): level 0 by the reference's push-order
    # Bellman-Ford from unsorted seeds (ns/lib/graph.py:40-51), relabelled in seed order
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, strength_mode="invabs", max_coarse=2000,
                                     aggregation="reference", coarse_order="sorted")
    assert H.n_levels == 5
    levels, Ac = oracle.build_hierarchy(A, alpha=0.1, strength_mode="invabs", max_coarse=2000,
                                        omegas=[L.omega for L in H.levels],
                                        aggregation="reference", coarse_order="sorted")
    assert len(levels) == len(H.levels)
    for l, (Lo, Ld) in enumerate(zip(levels, H.levels)):
        assert np.array_equal(Ld.seeds, Lo["seeds"]), l
        for key, M in (("P", Ld.P), ("A", Ld.A)):
            Md = M.to_scipy()
            for arr in ("indptr", "indices", "data"):
                assert np.array_equal(getattr(Md, arr), getattr(Lo[key], arr)), (l, key, arr)
            del Md
        assert np.array_equal(Ld.dinv.cpu().numpy(), Lo["Dw"].diagonal()), l
        f = {k: v for k, v in zip("APR", (Ld.A.get_format(), Ld.P.get_format(),
                                          Ld.R.get_format()))}
        for k, v in f.items():
            Lo[f"{k}_vw"] = v[1] if v[0] == "vector" else 0
        Lo["R"] = Lo["P"].T.tocsr()
        gc.collect()
    Acd = H.Ac.to_scipy()
    assert np.array_equal(Acd.indptr, Ac.indptr) and np.array_equal(Acd.indices, Ac.indices)
    assert np.array_equal(Acd.data, Ac.data)
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    x0 /= np.linalg.norm(x0)
    b = np.zeros(n)
    xo, ho = oracle.vcycle_solve(levels, Ac, b, x0, 4)
    xd = dev(torch, x0)
    hd = H.cycle(dev(torch, b), xd, 4)
    assert len(hd) == 4
    assert np.allclose(hd, ho, rtol=1e-11, atol=0), (hd, ho)
    assert np.allclose(xd.cpu().numpy(), xo, rtol=0, atol=1e-10 * np.abs(xo).max())


def _pair_patterns(A):
    """Distinct row-pair patterns of the rowpat format and their merged entry counts."""
    n = A.shape[0]

    def row(i):
        if i >= n:
            return (), b""
        a, b = A.indptr[i], A.indptr[i + 1]
        return tuple(A.indices[a:b] - i), A.data[a:b].tobytes()

    pats = {}
    for i in range(0, n, 2):
        (o0, v0), (o1, v1) = row(i), row(i + 1)
        pats[(o0, v0, o1, v1)] = len(set(o0) | set(o1))
    # padded to whole kernel steps: the longest pattern when 5..8 entries, else 8
    mx = max(pats.values())
    k = 5 if mx <= 5 else (mx if mx <= 8 else 8)
    return len(pats), sum(-(-m // k) * k for m in pats.values())


def test_rowpat_format(ml, torch_cuda):
    """Row-pair pattern format: bitwise CSR order on stencils (3D, 2D with odd n so pairs
    straddle grid lines and the last pair is single), boundary rows and empty rows included,
    every epilogue through the hierarchy, a -0.0 entry kept apart, refusal (format unchanged)
    past 255 patterns, format bytes."""
    torch = torch_cuda
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError, call, ptr, stream_ptr
    rs = np.random.RandomState(11)
    for A in (ml.problems.poisson_3d_7pt(20), ml.problems.poisson_2d_5pt(37)):
        n = A.shape[0]
        npat, n_ent = _pair_patterns(A)
        x, b = rs.randn(n), rs.randn(n)
        xd, bd = dev(torch, x), dev(torch, b)
        Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("rowpat")
        assert Ad.get_format()[:2] == ("rowpat", npat)
        # pair ids + x + y, plus the pattern tables (k_rowpair) or the 256-entry mask table of
        # the uniform-stencil form (k_rowpat_uni, csrc/spmv.hip)
        assert Ad.format_bytes() in (16.0 * n + (n + 1) // 2 + 4 * 257 + 32 * n_ent,
                                     16.0 * n + (n + 1) // 2 + 2 * 256)
        assert np.array_equal(Ad.matvec(xd).cpu().numpy(), A @ x)
        r = torch.empty(n, dtype=torch.float64, device="cuda")
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), stream_ptr())
        assert np.array_equal(r.cpu().numpy(), b - A @ x)
        assert abs(nrm.item() - np.linalg.norm(b - A @ x)) <= 1e-13 * np.linalg.norm(b - A @ x)
        # misaligned vectors (8-byte aligned views): the scalar epilogue path, same bits
        xo = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        xo[1:] = xd
        yo = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        call("mlamg_spmv", Ad.handle, ptr(xo[1:]), ptr(yo[1:]), 1.0, 0.0, stream_ptr())
        assert np.array_equal(yo[1:].cpu().numpy(), A @ x)
    A = ml.problems.poisson_3d_7pt(20)
    n = A.shape[0]
    x = rs.randn(n)
    xd = dev(torch, x)
    # a -0.0 value and an emptied row make pair patterns of their own
    B = A.tolil()
    B[7, :] = 0
    B = B.tocsr()
    B.eliminate_zeros()
    B.data = B.data.copy()
    B.data[100] = -0.0
    Bd = ml.sparse.DeviceCSR.from_scipy(B).set_format("rowpat")
    assert Bd.get_format()[1] == _pair_patterns(B)[0]
    assert np.array_equal(Bd.matvec(xd).cpu().numpy(), B @ x)
    # > 255 patterns -> refused, format unchanged, still bitwise
    R = sp.random(2000, 2000, density=0.01, random_state=rs, format="csr")
    Rd = ml.sparse.DeviceCSR.from_scipy(R).set_format("sell")
    with pytest.raises(MlamgError) as ei:
        Rd.set_format("rowpat")
    assert ei.value.code == MLAMG_EUNSUPPORTED
    assert Rd.get_format()[0] == "sell"
    xr = rs.randn(2000)
    assert np.array_equal(Rd.matvec(dev(torch, xr)).cpu().numpy(), R @ xr)
    # whole cycle with the fine operator as row-pair patterns == all-CSR-stream cycle
    b = rs.randn(n)
    bd = dev(torch, b)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream")
    H2 = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=100, fine_format="csr_stream")
    H2.levels[0].A.set_format("rowpat")
    x1, x2 = dev(torch, x), dev(torch, x)
    h1 = H.cycle(bd, x1, 5)
    h2 = H2.cycle(bd, x2, 5)
    assert torch.equal(x1, x2)
    assert np.allclose(h1, h2, rtol=1e-14, atol=0)
    # attached Jacobi weights (per-pattern constants from the table): the same bits, eager and
    # through the re-captured graph
    A2 = H2.levels[0].A
    assert A2.attach_dinv(H2.levels[0].dinv)
    for use_graph in (False, True):
        x1, x2 = dev(torch, x), dev(torch, x)
        h1 = H.cycle(bd, x1, 5, use_graph=use_graph)
        h2 = H2.cycle(bd, x2, 5, use_graph=use_graph)
        assert torch.equal(x1, x2)
        assert np.allclose(h1, h2, rtol=1e-14, atol=0)
    # weights that are not constant over the patterns are refused (nothing attached)
    d2 = H2.levels[0].dinv.clone()
    d2[5] *= 2.0
    assert not A2.attach_dinv(d2)
    y1 = torch.empty(n, dtype=torch.float64, device="cuda")
    y2 = torch.empty(n, dtype=torch.float64, device="cuda")
    t1 = torch.empty_like(y1)
    xs = dev(torch, x)
    call("mlamg_jacobi", A2.handle, ptr(d2), ptr(bd), ptr(xs), ptr(t1), 1, stream_ptr())
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    xs2 = dev(torch, x)
    call("mlamg_jacobi", Ad.handle, ptr(d2), ptr(bd), ptr(xs2), ptr(t1), 1, stream_ptr())
    assert torch.equal(xs, xs2)


@pytest.mark.parametrize("win", ["1", "0"])
def test_rowpat_window(ml, torch_cuda, monkeypatch, win):
    """Row-pair kernel with the LDS row window (k_rowpair_win, opt-in MLAMG_RP_WIN=1) and
    without (k_rowpair, the default): bitwise scipy for y = A x, the residual, Jacobi with xin == x (window
    operand) and xin != x, the cycle's fused end residual; 48^3 puts the +-n^2 entries beyond the
    largest halo (global loads beside window reads), 24^3 and 2D 37^2 keep them all in it."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    monkeypatch.setenv("MLAMG_RP_WIN", win)
    rs = np.random.RandomState(12)
    for A in (ml.problems.poisson_3d_7pt(48), ml.problems.poisson_3d_7pt(24),
              ml.problems.poisson_2d_5pt(37)):
        n = A.shape[0]
        x, b, d = rs.randn(n), rs.randn(n), rs.rand(n) + 0.5
        xd, bd, dd = dev(torch, x), dev(torch, b), dev(torch, d)
        Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("rowpat")
        y = A @ x
        assert np.array_equal(Ad.matvec(xd).cpu().numpy(), y)
        r = torch.empty(n, dtype=torch.float64, device="cuda")
        call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), None, stream_ptr())
        assert np.array_equal(r.cpu().numpy(), b - y)
        xs = dev(torch, x)
        t = torch.empty_like(xs)
        call("mlamg_jacobi", Ad.handle, ptr(dd), ptr(bd), ptr(xs), ptr(t), 1, stream_ptr())
        assert np.array_equal(xs.cpu().numpy(), x + d * (b - y))
    A = ml.problems.poisson_3d_7pt(48)
    bd = dev(torch, rs.randn(A.shape[0]))
    x0 = rs.randn(A.shape[0])
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, fine_format="csr_stream")
    H2 = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, fine_format="csr_stream")
    H2.levels[0].A.set_format("rowpat")
    assert H2.levels[0].A.attach_dinv(H2.levels[0].dinv)
    for use_graph in (False, True):
        x1, x2 = dev(torch, x0), dev(torch, x0)
        h1 = H.cycle(bd, x1, 4, use_graph=use_graph)
        h2 = H2.cycle(bd, x2, 4, use_graph=use_graph)
        assert torch.equal(x1, x2)
        assert np.allclose(h1, h2, rtol=1e-14, atol=0)


@pytest.mark.parametrize("rpm,ch,seg,pf", [
    ("1", "4", "0", "1"), ("1", "4", "1", "1"), ("1", "2", "0", "1"), ("1", "2", "3", "1"),
    ("1", "4", "7", "1"), ("1", "1", "0", "1"), ("1", "2", "0", "2"), ("1", "1", "3", "2"),
    ("1", "2", "1", "2"), ("0", "4", "0", "1")])
def test_rowpat_march(ml, torch_cuda, monkeypatch, rpm, ch, seg, pf):
    """Plane-marching form of the uniform 3-D stencil kernel (k_rowpat_march, csrc/spmv.hip;
    MLAMG_RPM=0: k_rowpat_uni): every non-norm epilogue bitwise scipy — y = A x, y = 2 A x -
    y/2, the residual, Jacobi (xin == x, window operand; nu = 2; attached weights), the explicit
    form, x += A e — on planes that are a whole number of tiles (64^3), a partial last tile
    (48^3, 46^3), an odd plane (47^3: not marched), segments of 1, 3, 7 planes or the
    automatic length, and one or two planes prefetched; the norm form (k_rowpat_uni) alongside; the cycle equals the
    CSR-stream cycle bit for bit, eager and from the captured graph."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    monkeypatch.setenv("MLAMG_RPM", rpm)
    monkeypatch.setenv("MLAMG_RPM_CH", ch)
    monkeypatch.setenv("MLAMG_RPM_SEG", seg)
    monkeypatch.setenv("MLAMG_RPM_PF", pf)
    rs = np.random.RandomState(13)
    s = stream_ptr()
    for m in (64, 48, 46, 47):
        A = ml.problems.poisson_3d_7pt(m)
        n = A.shape[0]
        x, b, d, y0 = rs.randn(n), rs.randn(n), rs.rand(n) + 0.5, rs.randn(n)
        xd, bd, dd = dev(torch, x), dev(torch, b), dev(torch, d)
        Ad = ml.sparse.DeviceCSR.from_scipy(A).set_format("rowpat")
        y = A @ x
        assert np.array_equal(Ad.matvec(xd).cpu().numpy(), y)
        yd = dev(torch, y0)
        call("mlamg_spmv", Ad.handle, ptr(xd), ptr(yd), 2.0, -0.5, s)
        assert np.array_equal(yd.cpu().numpy(), 2.0 * y + (-0.5) * y0)
        r = torch.empty(n, dtype=torch.float64, device="cuda")
        call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), None, s)
        assert np.array_equal(r.cpu().numpy(), b - y)
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        r.zero_()
        call("mlamg_residual", Ad.handle, ptr(bd), ptr(xd), ptr(r), ptr(nrm), s)
        assert np.array_equal(r.cpu().numpy(), b - y)
        assert abs(nrm.item() - np.linalg.norm(b - y)) <= 1e-13 * np.linalg.norm(b - y)
        xs, t = dev(torch, x), torch.empty(n, dtype=torch.float64, device="cuda")
        call("mlamg_jacobi", Ad.handle, ptr(dd), ptr(bd), ptr(xs), ptr(t), 2, s)
        x1 = x + d * (b - y)
        assert np.array_equal(xs.cpu().numpy(), x1 + d * (b - A @ x1))
        xs = dev(torch, x)
        call("mlamg_jacobi_explicit", Ad.handle, ptr(dd), ptr(bd), ptr(xs), ptr(t), 1, s)
        assert np.array_equal(xs.cpu().numpy(), x + (d * b - y))
        xs = dev(torch, y0)
        call("mlamg_prolong_add", Ad.handle, ptr(xd), ptr(xs), s)
        assert np.array_equal(xs.cpu().numpy(), y0 + y)
        # attached weights (the per-pattern table) give the same bits
        dw = dev(torch, np.full(n, 1.0 / 9.0))
        assert Ad.attach_dinv(dw)
        xs = dev(torch, x)
        call("mlamg_jacobi", Ad.handle, ptr(dw), ptr(bd), ptr(xs), ptr(t), 1, s)
        assert np.array_equal(xs.cpu().numpy(), x + np.full(n, 1.0 / 9.0) * (b - y))
    A = ml.problems.poisson_3d_7pt(48)
    bd = dev(torch, rs.randn(A.shape[0]))
    x0 = rs.randn(A.shape[0])
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, fine_format="csr_stream")
    H2 = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, fine_format="csr_stream")
    H2.levels[0].A.set_format("rowpat")
    assert H2.levels[0].A.attach_dinv(H2.levels[0].dinv)
    for use_graph in (False, True):
        x1, x2 = dev(torch, x0), dev(torch, x0)
        h1 = H.cycle(bd, x1, 4, use_graph=use_graph)
        h2 = H2.cycle(bd, x2, 4, use_graph=use_graph)
        assert torch.equal(x1, x2)
        assert np.allclose(h1, h2, rtol=1e-14, atol=0)


def test_supplied_aggregates_and_prolongator(ml, oracle, torch_cuda):
    """Hierarchy.build with supplied level-0 aggregates (C5: learned/supplied aggregates on the
    jump-coefficient problem) and with a supplied P (the MLAMG PC's learned P,
    ns/preconditioner/MLAMG.py:105-121): level-0 P = the oracle's SA prolongator of those
    aggregates with the device omega (bitwise) / the given P itself; the cycle matches the
    oracle's on the device's operators."""
    torch = torch_cuda
    m = 48
    A = ml.problems.jump_2d(m, ml.problems.voronoi_jumps(np.random.RandomState(0)))
    Agg = ml.problems.box_aggregates_2d(m, m, 3)
    labels = np.asarray(Agg.argmax(axis=1)).ravel()
    for spec in (labels, Agg):
        H = ml.hierarchy.Hierarchy.build(A, aggregates=spec, max_coarse=60)
        assert H.levels[0].n_seeds == Agg.shape[1]
        P_ref, _ = oracle.smoothed_aggregation_jacobi(A, Agg, omega=H.levels[0].omega)
        Pd = H.levels[0].P.to_scipy()
        assert np.array_equal(Pd.indptr, P_ref.indptr) and np.array_equal(Pd.data, P_ref.data)
    lv = _oracle_levels_from_device(H)
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    b = np.random.RandomState(1).randn(n)
    xo, ho = oracle.vcycle_solve(lv, H.Ac.to_scipy(), b, x0, 5)
    xd = dev(torch, x0)
    hd = H.cycle(dev(torch, b), xd, 5)
    assert np.allclose(hd, ho, rtol=1e-11, atol=0)
    # a supplied P is used as given (no smoothing)
    H2 = ml.hierarchy.Hierarchy.build(A, prolongators=[P_ref], max_levels=2)
    P2 = H2.levels[0].P.to_scipy()
    assert np.array_equal(P2.data, P_ref.data) and np.array_equal(P2.indices, P_ref.indices)
    with pytest.raises(ValueError):
        ml.hierarchy.Hierarchy.build(A, aggregates=labels[:-1])


def test_autotune_cache_reuses_decisions(ml, torch_cuda):
    """The format autotune keeps its decision per operator fingerprint (rows, columns, value
    bits): a hierarchy rebuilt on the same operator takes the same kernels without re-timing
    (VERDICT r04 Next #7), and an operator with one value changed is timed afresh."""
    torch = torch_cuda
    H_ = ml.hierarchy.Hierarchy
    H_.clear_tune_cache()
    A = ml.problems.poisson_2d_5pt(200)
    H1 = H_.build(A, alpha=0.1, max_coarse=300)
    assert not any(r.get("cached") for row in H1.tuning for r in row.values())
    H2 = H_.build(A, alpha=0.1, max_coarse=300)
    assert all(r.get("cached") for row in H2.tuning for r in row.values())
    assert H1.formats() == H2.formats()
    assert H2.timings["formats"] < H1.timings["formats"]
    b = torch.zeros(A.shape[0], dtype=torch.float64, device="cuda")
    x0 = np.random.RandomState(0).randn(A.shape[0])
    h1 = H1.cycle(b, dev(torch, x0), 4)
    h2 = H2.cycle(b, dev(torch, x0), 4)
    assert np.array_equal(h1, h2)
    A2 = A.copy()
    A2.data[0] *= 1.0 + 2.0 ** -40
    H3 = H_.build(A2, alpha=0.1, max_coarse=300)
    assert not H3.tuning[0]["A"].get("cached")
    Ad = ml.sparse.DeviceCSR.from_scipy(A)
    assert Ad.fingerprint() == ml.sparse.DeviceCSR.from_scipy(A).fingerprint()
    assert Ad.fingerprint() != ml.sparse.DeviceCSR.from_scipy(A2).fingerprint()


def test_zero_rhs_same_bits(ml, torch_cuda):
    """A zero right-hand side (the reference's conv-factor problems, b = zeros) is passed to the
    cycle as NULL (hierarchy.rhs_arg): the fine-level kernels take b = +0.0 instead of streaming
    zeros. Iterates and histories are bitwise those of the streamed-b kernels — multilevel
    Jacobi (graph and eager, with and without a tolerance), the two-level Gauss-Seidel cycle
    (zero buffer), and a coarse-only hierarchy; a -0.0 entry is not a zero right-hand side."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    from mlamg.hierarchy import rhs_arg
    A = ml.problems.poisson_3d_7pt(30)
    n = A.shape[0]
    x0 = np.random.RandomState(4).randn(n)
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=300)
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert rhs_arg(b) is None
    bm = b.clone()
    bm[7] = -0.0
    assert rhs_arg(bm) is bm
    for use_graph in (True, False):
        for tol in (None, 1e-6):
            x1 = dev(torch, x0)
            h1 = H.cycle(b, x1, 8, tol=tol, use_graph=use_graph)  # detected: NULL b
            x2 = dev(torch, x0)
            hist = torch.zeros(8, dtype=torch.float64, device="cuda")
            done = ctypes.c_int32()
            call("mlamg_hier_vcycle", H.handle, ptr(b), ptr(x2), 8,
                 -1.0 if tol is None else tol, ptr(hist), ctypes.byref(done), int(use_graph),
                 stream_ptr())  # b streamed
            h2 = hist[: done.value].cpu().numpy()
            assert np.array_equal(h1, h2) and torch.equal(x1, x2), (use_graph, tol)
    x3 = dev(torch, x0)
    H.cycle_async(b, x3, 8, zero_rhs=False)
    x4 = dev(torch, x0)
    H.cycle_async(b, x4, 8, zero_rhs=True)
    assert torch.equal(x3, x4)
    with pytest.raises(ValueError):
        H.cycle_async(bm + 1.0, x4, 1, zero_rhs=True)
    # two-level Gauss-Seidel (multigrid.amg_2_v's cycle) and a coarse-only hierarchy
    P = H.levels[0].P.to_scipy()
    for smoother in ("gauss_seidel", "jacobi"):
        H2 = ml.hierarchy.Hierarchy.two_level(A, P, smoother=smoother)
        xa, xb = dev(torch, x0), dev(torch, x0)
        ha = H2.cycle(b, xa, 5)
        hb = torch.zeros(5, dtype=torch.float64, device="cuda")
        call("mlamg_hier_vcycle", H2.handle, ptr(b), ptr(xb), 5, -1.0, ptr(hb), None, 1,
             stream_ptr())
        assert np.array_equal(ha, hb.cpu().numpy()) and torch.equal(xa, xb), smoother
    small = ml.problems.poisson_2d_5pt(20)
    Hc = ml.hierarchy.Hierarchy.build(small, alpha=0.1, max_coarse=1000)
    assert Hc.n_levels == 1
    xc = dev(torch, np.ones(small.shape[0]))
    Hc.cycle(torch.zeros(small.shape[0], dtype=torch.float64, device="cuda"), xc, 1)
    assert float(xc.abs().max()) == 0.0


@pytest.mark.parametrize("dim,n1", ((3, 40), (2, 201)))
def test_factored_prolongation_within_tolerance(ml, oracle, torch_cuda, dim, n1):
    """Opt-in factored level-0 prolongation (VERDICT r04 Next #5): x += t - (w/a_ii) A t with
    t = Agg e instead of x += P e (ns/lib/multigrid.py:102-108's P = (I - w D^-1 A) Agg,
    applied without streaming P). Not bitwise the explicit P: the residual history stays
    within rtol 1e-11 of the oracle's cycle on the explicit operators, and the iterate within
    1e-10 of its max; off again, the cycle is the explicit one bit for bit. The 3-D 7-point and
    an odd 2-D grid (an odd row count: the row-pair window's last pair single)."""
    torch = torch_cuda
    A = ml.problems.poisson_3d_7pt(n1) if dim == 3 else ml.problems.poisson_2d_5pt(n1)
    n = A.shape[0]
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=500, aggregation="reference",
                                     coarse_order="sorted")
    if H.levels[0].A.get_format()[0] != "rowpat":  # the autotune's pick; any exact format
        H.levels[0].A.set_format("rowpat")        # computes the same bits
        H.attach_dinvs()
    lv = []
    for L in H.levels:
        f = {k: M.get_format() for k, M in (("A", L.A), ("P", L.P), ("R", L.R))}
        vw = {k: (v[1] if v[0] == "vector" else 0) for k, v in f.items()}
        lv.append({"A": L.A.to_scipy(), "P": L.P.to_scipy(), "R": L.R.to_scipy(),
                   "Dw": sp.diags(L.dinv.cpu().numpy()),
                   "A_vw": vw["A"], "P_vw": vw["P"], "R_vw": vw["R"]})
    x0 = np.random.RandomState(0).randn(n)
    b = np.random.RandomState(1).randn(n)
    xo, ho = oracle.vcycle_solve(lv, H.Ac.to_scipy(), b, x0, 6)
    xe = dev(torch, x0)
    he = H.cycle(dev(torch, b), xe, 6)
    assert np.allclose(he, ho, rtol=1e-11, atol=0)
    H.set_factored_prolong(0)
    xf = dev(torch, x0)
    hf = H.cycle(dev(torch, b), xf, 6)
    assert np.allclose(hf, ho, rtol=1e-11, atol=0), (hf, ho)
    assert np.allclose(xf.cpu().numpy(), xo, rtol=0, atol=1e-10 * np.abs(xo).max())
    # zero right-hand side (the bench's problem) too
    z = torch.zeros(n, dtype=torch.float64, device="cuda")
    xz = dev(torch, x0)
    hz = H.cycle(z, xz, 6)
    _, hoz = oracle.vcycle_solve(lv, H.Ac.to_scipy(), np.zeros(n), x0, 6)
    assert np.allclose(hz, hoz, rtol=1e-11, atol=0)
    H.set_factored_prolong(0, on=False)
    x2 = dev(torch, x0)
    h2 = H.cycle(dev(torch, b), x2, 6)
    assert np.array_equal(h2, he) and torch.equal(x2, xe)
    # a hierarchy whose operator has no uniform stencil refuses it
    Hv = ml.hierarchy.Hierarchy.build(ml.problems.random_coeff_3d_7pt(20, seed=0), alpha=0.1,
                                      max_coarse=500)
    from mlamg._lib import MlamgError
    with pytest.raises(MlamgError):
        Hv.set_factored_prolong(0)


@pytest.mark.parametrize("case,fmt", [("p3d", ("rowpat", 0)), ("p3d", ("sorted", 0)),
                                      ("p3d", ("sell", 1)), ("p3d", ("sell_dict", 1)),
                                      ("p3d", ("csr_stream", 0)), ("p2d_1536", ("csr_stream", 0)),
                                      ("varcoef", ("sell", 512)), ("varcoef", ("sorted", 0)),
                                      ("varcoef", ("sorted", 2))])
def test_end_of_cycle_norm_same_bits(ml, torch_cuda, case, fmt):
    """The end-of-cycle norm of the fused cycle (the residual pass of t that also writes the next
    cycle's first sweep, MLAMG.py:194) is the norm mlamg_residual computes on the same iterate:
    after one cycle x holds t and hist[0] = ||b - A t|| bit for bit. Every fine-level format, up
    to 9,216 norm partials (k_finalize_norm's unrolled strided loop); then a tolerance stop on
    the cycle whose norm met it."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    if case == "p3d":
        A = ml.problems.poisson_3d_7pt(40)
    elif case == "p2d_1536":
        A = ml.problems.poisson_2d_5pt(1536)
    else:
        A = ml.problems.random_coeff_3d_7pt(40, seed=1)
    n = A.shape[0]
    H = ml.hierarchy.Hierarchy.build(A, alpha=0.1, max_coarse=2000)
    try:
        H.levels[0].A.set_format(*fmt)
    except ml._lib.MlamgError as e:
        # the per-block dictionary refuses random coefficients (more than half of a block's
        # values distinct): that refusal is the expected outcome, and the only one
        assert e.code == ml._lib.MLAMG_EUNSUPPORTED and (case, fmt) == ("varcoef", ("sorted", 2)), e
        return
    H.attach_dinvs()
    rng = np.random.RandomState(3)
    b = dev(torch, rng.randn(n))
    x = dev(torch, rng.randn(n))
    for k in range(3):
        h = H.cycle(b, x, 1)
        r = torch.empty_like(x)
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        call("mlamg_residual", H.levels[0].A.handle, ptr(b), ptr(x), ptr(r), ptr(nrm),
             stream_ptr())
        assert h[0] == float(nrm[0]), (k, h[0], float(nrm[0]))
    x1 = dev(torch, rng.randn(n))
    x2 = x1.clone()
    h_all = H.cycle(b, x1, 12)
    tol = float(h_all[6])  # met first by cycle 7
    h_tol = H.cycle(b, x2, 12, tol=tol)
    assert len(h_tol) == 7 and np.array_equal(h_tol, h_all[:7])
