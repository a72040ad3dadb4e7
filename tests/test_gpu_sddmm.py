"""GPU: mlamg_sddmm / DeviceCSR.sddmm, the sampled dense-dense product on a CSR pattern
(csrc/sddmm.hip): out[e] = alpha * (U[row(e), :] . V[col(e), :]) + beta * out[e].

The summation order is part of the contract (include/mlamg.h): `restate` below is that order in
numpy, and every result is compared with it by np.array_equal. The accuracy bound against a
np.longdouble dot product is the standard one for a k-term fp64 sum in any order,
gamma_k sum_c |U[i,c] V[j,c]| with gamma_k = k u / (1 - k u), u = 2^-53, doubled for the rounding
of the reference's own result to fp64: derived, not measured."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 17, 64)
PATTERNS = ("sa_P_576x64", "poisson_576", "random_300x40", "long_row_300x2600")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.problems
    import mlamg.sparse
    return mlamg


def _random_pattern(n_rows, n_cols, seed, long_row=None):
    """Rows of 0..5 entries (so some are empty), the last row empty; long_row = (row, count)
    gives one row `count` entries."""
    rs = np.random.RandomState(seed)
    S = sp.lil_matrix((n_rows, n_cols))
    for i in range(n_rows - 1):
        m = rs.randint(0, 6)
        S[i, rs.choice(n_cols, size=m, replace=False)] = 1.0
    if long_row is not None:
        S[long_row[0], :] = 0.0
        S[long_row[0], rs.choice(n_cols, size=long_row[1], replace=False)] = 1.0
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return S


@pytest.fixture(scope="module")
def patterns(ml):
    m = 24
    A = ml.problems.poisson_2d_5pt(m).tocsr()
    agg = sp.csr_matrix(ml.problems.box_aggregates_2d(m, m, 3))
    Dinv = sp.diags([1.0 / A.diagonal()], [0])
    P = sp.csr_matrix((sp.eye(m * m) - (2.0 / 3.0) * Dinv @ A) @ agg)
    P.sort_indices()
    out = {"sa_P_576x64": P, "poisson_576": A,
           "random_300x40": _random_pattern(300, 40, 11),
           "long_row_300x2600": _random_pattern(300, 2600, 12, long_row=(7, 2500))}
    assert out["sa_P_576x64"].shape == (576, 64)
    lens = np.diff(out["random_300x40"].indptr)
    assert lens[-1] == 0 and (lens[:-1] == 0).any()
    lens = np.diff(out["long_row_300x2600"].indptr)
    assert lens[7] == 2500 and lens[-1] == 0 and (lens == 0).sum() > 1
    return {name: (S, ml.sparse.DeviceCSR.from_scipy(S)) for name, S in out.items()}


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


def _rows_cols(S):
    return np.repeat(np.arange(S.shape[0]), np.diff(S.indptr)), S.indices


def restate(S, U, V, alpha=1.0, beta=0.0, out0=None):
    """The documented order: pairs of adjacent columns, then a pairwise tree over the
    G = next_pow2(ceil(k/2)) pair sums (columns >= k are +0.0); alpha and beta applied with
    separate roundings, out0 not read when beta == 0."""
    k = U.shape[1]
    G = 1
    while G < (k + 1) // 2:
        G *= 2
    rows, cols = _rows_cols(S)
    Up = np.zeros((U.shape[0], 2 * G))
    Vp = np.zeros((V.shape[0], 2 * G))
    Up[:, :k] = U
    Vp[:, :k] = V
    prod = Up[rows] * Vp[cols]
    t = prod[:, 0::2] + prod[:, 1::2]
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    s = t[:, 0]
    if beta == 0.0:
        return alpha * s
    a = alpha * s
    b = beta * out0
    return a + b


def _blocks(S, k, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((S.shape[0], k)), rs.standard_normal((S.shape[1], k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_bits_and_bound(torch_cuda, patterns, name, k):
    torch = torch_cuda
    S, Sd = patterns[name]
    U, V = _blocks(S, k, 100 + k)
    got = host(Sd.sddmm(dev(torch, U), dev(torch, V)))
    assert got.shape == (S.nnz,)
    assert np.array_equal(got, restate(S, U, V)), (name, k)
    rows, cols = _rows_cols(S)
    ref = (U[rows].astype(np.longdouble) * V[cols].astype(np.longdouble)).sum(axis=1)
    mag = np.abs(U[rows] * V[cols]).sum(axis=1)
    u = 2.0 ** -53
    gamma = k * u / (1.0 - k * u)
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print(f"{name} k={k}: max err / (gamma_k sum|uv|) = {(err / (gamma * mag)).max():.3f}")
    assert np.all(err <= 2.0 * gamma * mag), (name, k)
    # two launches: identical bits
    again = host(Sd.sddmm(dev(torch, U), dev(torch, V)))
    assert np.array_equal(got, again)


@pytest.mark.parametrize("k", (3, 8, 17))
@pytest.mark.parametrize("name", ("sa_P_576x64", "long_row_300x2600"))
def test_sddmm_strides_and_instantiations(torch_cuda, patterns, name, k):
    """U and V as column slices at an odd column offset of buffers with an odd leading
    dimension (rows not 16-byte aligned: the 8-byte instantiation) and at offset 0 of buffers
    with an even one (the 16-byte instantiation): the same bits, the restatement's."""
    torch = torch_cuda
    S, Sd = patterns[name]
    U, V = _blocks(S, k, 7)
    want = restate(S, U, V)

    def sliced(a, width, off):
        buf = torch.full((a.shape[0], width), 3.25, dtype=torch.float64, device="cuda")
        buf[:, off:off + k] = dev(torch, a)
        return buf[:, off:off + k]

    w_odd = k + 2 if k % 2 else k + 3
    w_even = k + 1 if k % 2 else k
    Us, Vs = sliced(U, w_odd, 1), sliced(V, w_odd + 2, 1)
    assert Us.stride(0) % 2 == 1 and Vs.stride(0) % 2 == 1 and Us.data_ptr() % 16 == 8
    Uv, Vv = sliced(U, w_even, 0), sliced(V, w_even + 2, 0)
    assert Uv.stride(0) % 2 == 0 and Vv.stride(0) % 2 == 0
    assert Uv.data_ptr() % 16 == 0 and Vv.data_ptr() % 16 == 0
    scalar = host(Sd.sddmm(Us, Vs))
    vec = host(Sd.sddmm(Uv, Vv))
    assert np.array_equal(scalar, vec)
    assert np.array_equal(vec, want)
    # one aligned, one not: still the same bits
    assert np.array_equal(host(Sd.sddmm(Uv, Vs)), want)


@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_alpha_beta(torch_cuda, patterns, name):
    torch = torch_cuda
    S, Sd = patterns[name]
    k = 6
    U, V = _blocks(S, k, 21)
    Ud, Vd = dev(torch, U), dev(torch, V)
    out = torch.full((S.nnz,), np.nan, dtype=torch.float64, device="cuda")
    res = Sd.sddmm(Ud, Vd, alpha=1.0, beta=0.0, out=out)  # beta == 0: out is not read
    assert res.data_ptr() == out.data_ptr()
    assert np.array_equal(host(out), restate(S, U, V))
    out0 = np.random.RandomState(22).standard_normal(S.nnz)
    for alpha, beta in ((-0.5, 1.0), (2.0, 0.25)):
        o = dev(torch, out0)
        Sd.sddmm(Ud, Vd, alpha=alpha, beta=beta, out=o)
        assert np.array_equal(host(o), restate(S, U, V, alpha, beta, out0)), (alpha, beta)
    o = torch.full((S.nnz,), np.nan, dtype=torch.float64, device="cuda")
    Sd.sddmm(Ud, Vd, alpha=3.0, out=o)
    assert np.array_equal(host(o), restate(S, U, V, 3.0))


def test_sddmm_reads_the_csr_arrays_whatever_the_format(torch_cuda, patterns, ml):
    torch = torch_cuda
    S, _ = patterns["poisson_576"]
    Sd = ml.sparse.DeviceCSR.from_scipy(S)
    U, V = _blocks(S, 8, 5)
    want = restate(S, U, V)
    for fmt in ("csr_stream", "sell", "sorted"):
        Sd.set_format(fmt)
        assert np.array_equal(host(Sd.sddmm(dev(torch, U), dev(torch, V))), want), fmt


def test_sddmm_wrapper_refusals(torch_cuda, patterns):
    torch = torch_cuda
    S, Sd = patterns["sa_P_576x64"]
    U, V = (dev(torch, a) for a in _blocks(S, 4, 1))
    with pytest.raises(ValueError):
        Sd.sddmm(U, V[:, :3])
    with pytest.raises(ValueError):
        Sd.sddmm(V, U)  # row counts swapped
    with pytest.raises(ValueError):
        Sd.sddmm(U, V, beta=1.0)  # nothing to accumulate into
    with pytest.raises(TypeError):
        Sd.sddmm(U, V, out=torch.zeros(S.nnz - 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        Sd.sddmm(U.cpu(), V)
    wide = torch.ones((S.shape[0], 65), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        Sd.sddmm(wide, torch.ones((S.shape[1], 65), dtype=torch.float64, device="cuda"))
