"""GPU: the block-diagonal dense coarse solve (mlamg_blockdense; csrc/blockdense.hip, DESIGN.md
§24). All blocks live in one handle. For every block mlamg_blockdense_info reports the method
mlamg_dense_info reports for that block alone, and the block's rows of a solve are bitwise
mlamg_dense_solve_mv of a handle created on that block alone.

Blocks: SPD of 1, 3, 63 (Gauss-Jordan: below 64 rows), 64, 65, 130 and 520 rows (inverse Cholesky
factor; 520 rows are a second lane batch of the row reduction and 17 Cholesky panels); a
non-symmetric block of 40 rows whose leading diagonal entry is zero (row interchanges) and one of
81 rows (>= 64: falls through from Cholesky to Gauss-Jordan, in LDS); a symmetric indefinite block
of 70 rows (the Cholesky pivot fails)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _spd(rng, n):
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n)


def _blocks():
    rng = np.random.default_rng(24)
    out = [("spd", _spd(rng, n), 0 if n < 64 else 1) for n in (1, 3, 63, 64, 65, 130, 520)]
    N = rng.standard_normal((40, 40)) + 3.0 * np.eye(40)
    N[0, 0] = 0.0  # the first pivot must come from another row
    out.append(("nonsym40", N, 0))
    out.append(("nonsym81", rng.standard_normal((81, 81)) + 9.0 * np.eye(81), 0))
    S = rng.standard_normal((70, 70))
    S = S + S.T + np.diag(np.where(np.arange(70) % 2 == 0, -20.0, 20.0))
    assert np.array_equal(S, S.T) and S[0, 0] < 0
    out.append(("indefinite70", S, 0))
    # both sides of every size at which the batched Gauss-Jordan changes its kernel: the LDS
    # tiers of 16, 32, 64 (63 and 81 above) and 128 rows, and the in-place variant beyond
    for n in (16, 17, 32, 33, 128, 129, 150):
        N = rng.standard_normal((n, n)) + np.sqrt(n) * np.eye(n)
        N[n // 2, n // 2] = 0.0
        out.append((f"nonsym{n}", N, 0))
    return out


@pytest.fixture(scope="module")
def setup(torch_cuda):
    """The stacked handle and, per block, a dense handle created on that block alone."""
    from mlamg._lib import call, lib, stream_ptr
    from mlamg.loss import BlockDense
    from mlamg.sparse import DeviceCSR
    blocks = _blocks()
    off = np.concatenate([[0], np.cumsum([b[1].shape[0] for b in blocks])]).astype(np.int64)
    stack = DeviceCSR.from_scipy(sp.block_diag([sp.csr_matrix(b[1]) for b in blocks],
                                               format="csr"))
    bd = BlockDense(stack, off)
    singles = []
    for _, M, _ in blocks:
        h = ctypes.c_void_p()
        Mc = DeviceCSR.from_scipy(sp.csr_matrix(M))
        call("mlamg_dense_create", Mc.handle, ctypes.byref(h), stream_ptr())
        singles.append(h)
    yield blocks, off, bd, singles
    for h in singles:
        lib.mlamg_dense_destroy(h)


def test_methods_are_the_single_calls(setup):
    from mlamg._lib import call
    blocks, off, bd, singles = setup
    got = bd.methods()
    nb, n = ctypes.c_int64(), ctypes.c_int64()
    call("mlamg_blockdense_info", bd.handle, ctypes.byref(nb), ctypes.byref(n), None)
    assert (nb.value, n.value) == (len(blocks), int(off[-1]))
    for i, (name, M, expect) in enumerate(blocks):
        m = ctypes.c_int()
        call("mlamg_dense_info", singles[i], ctypes.byref(m), None)
        assert got[i] == m.value == expect, (name, M.shape[0], got[i], m.value)


@pytest.mark.parametrize("k", KS)
def test_solve_is_bitwise_the_single_solve_per_block(torch_cuda, setup, k):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    blocks, off, bd, singles = setup
    n = int(off[-1])
    g = torch.Generator(device="cuda").manual_seed(7 + k)
    B = torch.randn((n, k), generator=g, dtype=torch.float64, device="cuda")
    X = bd.solve(B, torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")).cpu().numpy()
    for i, (name, M, _) in enumerate(blocks):
        a, b = int(off[i]), int(off[i + 1])
        Bi = B[a:b].clone().contiguous()
        Xi = torch.empty_like(Bi)
        call("mlamg_dense_solve_mv", singles[i], ptr(Bi), k, ptr(Xi), k, k, stream_ptr())
        assert np.array_equal(X[a:b], Xi.cpu().numpy()), (name, M.shape[0])
        # and it is a solve: the bitwise check alone would pass on two equal wrong answers
        ref = np.linalg.solve(M, Bi.cpu().numpy())
        assert np.allclose(X[a:b], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max()), name


def test_singular_block_and_stray_entry_are_named(torch_cuda):
    from mlamg._lib import MLAMG_EINVAL, MlamgError
    from mlamg.loss import BlockDense
    from mlamg.sparse import DeviceCSR
    rng = np.random.default_rng(3)
    good = [_spd(rng, 5), _spd(rng, 70), _spd(rng, 9)]
    # an exactly singular block: [[1, 2], [2, 4]] eliminates to an exact zero pivot
    mats = [good[0], np.array([[1.0, 2.0], [2.0, 4.0]]), good[1], good[2]]
    off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    A = sp.block_diag([sp.csr_matrix(m) for m in mats], format="csr")
    with pytest.raises(MlamgError, match="block 1 is exactly singular") as e:
        BlockDense(DeviceCSR.from_scipy(A), off)
    assert e.value.code == MLAMG_EINVAL
    # an entry outside the diagonal blocks, in row 80 (block 3) and column 2 (block 0)
    mats[1] = np.array([[1.0, 2.0], [2.0, 5.0]])
    A = sp.lil_matrix(sp.block_diag([sp.csr_matrix(m) for m in mats]))
    A[80, 2] = 1.0
    A[83, 1] = 1.0
    with pytest.raises(MlamgError, match="row 80 has an entry outside the diagonal blocks") as e:
        BlockDense(DeviceCSR.from_scipy(A.tocsr()), off)
    assert e.value.code == MLAMG_EINVAL
    # the same operator without the stray entries is accepted
    A[80, 2] = 0.0
    A[83, 1] = 0.0
    ok = A.tocsr()
    ok.eliminate_zeros()
    assert BlockDense(DeviceCSR.from_scipy(ok), off).methods() == [0, 0, 1, 0]
