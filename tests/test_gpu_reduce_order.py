"""The fixed reduction order (csrc/reduce.hpp), stated on the host and pinned bitwise.

Every other reduction test compares one kernel to another; this one compares the kernels to a
numpy transcription of the order itself (tests/reduce_order.py, shared with the LSQR model):
  1. thread t of workgroup b of a grid of G workgroups of NT threads adds the entries
     b*NT + t + m*G*NT, m ascending, to an accumulator that starts at +0.0;
  2. the 64-lane xor butterfly, offsets 32 .. 1, by lane index;
  3. the NT/64 wave totals added left to right;
  4. one workgroup sums the G partials: thread t takes the partials t, t + NT, .. in that order
     (strided_sum), then 2 and 3 again.
The sizes sit at the edges of a wave, a workgroup and a grid cap."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from reduce_order import (block_totals, ill_scaled, partials_total, remove_mean_ref,
                          sum_ref, sumsq_ref, thread_sums, wave_totals)

EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------- host
@pytest.mark.parametrize("n", (1, 257, 262145))
def test_transcription_sums_what_fsum_sums(n):
    """Any order of n additions is within (n - 1) u sum|v| of the exact sum, u = eps / 2: the
    transcription must be within n eps of math.fsum, relative to sum|v|."""
    x = ill_scaled(n, n)
    sq = x * x
    f = math.fsum(sq)
    assert abs(sumsq_ref(x) - f) <= n * EPS * f
    assert abs(sum_ref(x) - math.fsum(x)) <= n * EPS * math.fsum(np.abs(x))


@pytest.mark.parametrize("kind", ("random", "ill_scaled", "minus_zero"))
def test_four_wave_finish_spellings_agree(kind):
    """((r0 + r1) + r2) + r3 and t = 0.0; t += r[i] differ only for r0 = -0.0, which a wave
    total of accumulators that start at +0.0 never is."""
    n = 524289
    if kind == "random":
        x = np.random.RandomState(3).standard_normal(n)
    elif kind == "ill_scaled":
        x = ill_scaled(n, 4)
    else:
        x = np.full(n, -0.0)
    for vals, G in ((x, 512), (x * x, 1024)):
        r = wave_totals(thread_sums(vals, G, 256))
        assert not np.any((r == 0) & np.signbit(r))
        a = ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]
        b = np.zeros(G)
        for i in range(4):
            b = b + r[:, i]
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert np.array_equal(a.view(np.int64), block_totals(thread_sums(vals, G, 256)).view(np.int64))


# ---------------------------------------------------------------- device
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def lib(torch_cuda):
    import mlamg.sparse  # noqa: F401  (loads the library)
    from mlamg import _lib
    return _lib


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def vector(n, kind):
    if kind == "zero":
        return np.zeros(n)
    if kind == "minus_zero":
        return np.full(n, -0.0)
    return ill_scaled(n, n)


NORM_CASES = [(n, "ill") for n in (1, 63, 64, 65, 255, 256, 257, 1000, 262144, 262145)]
NORM_CASES += [(257, "zero"), (257, "minus_zero"), (262145, "minus_zero")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", NORM_CASES)
def test_norm2_is_the_stated_order(torch_cuda, lib, n, kind):
    torch = torch_cuda
    x = vector(n, kind)
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    xd = dev(torch, x)
    lib.call("mlamg_norm2", lib.ptr(xd), n, lib.ptr(out), lib.stream_ptr())
    got, ref = out.cpu().numpy(), np.sqrt(sumsq_ref(x))
    assert np.array_equal(bits(got), bits([ref]))


MEAN_CASES = [(n, "ill") for n in (1, 257, 131072, 131073)] + [(257, "minus_zero"),
                                                               (131073, "minus_zero")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", MEAN_CASES)
def test_remove_mean_is_the_stated_order(torch_cuda, lib, n, kind):
    torch = torch_cuda
    x = vector(n, kind)
    xd = dev(torch, x)
    lib.call("mlamg_remove_mean", lib.ptr(xd), n, lib.stream_ptr())
    got = xd.cpu().numpy()
    assert np.array_equal(bits(got), bits(remove_mean_ref(x)))
    if kind == "minus_zero":
        assert np.all(np.signbit(got)) and np.all(got == 0)  # -0.0 - (+0.0 / n) = -0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", (257, 262145))
def test_mv_columns_are_the_stated_order(torch_cuda, lib, n):
    """k = 9 columns (a full tile of 8 and a tile of 1) in a block of leading dimension 12."""
    torch = torch_cuda
    k, ld = 9, 12
    X = ill_scaled(n * ld, n + 1).reshape(n, ld)
    Xd = dev(torch, X)
    out = torch.full((ld,), -1.0, dtype=torch.float64, device="cuda")
    s = lib.stream_ptr()
    lib.call("mlamg_norm2_mv", lib.ptr(Xd), ld, n, k, lib.ptr(out), s)
    got = out.cpu().numpy()
    ref = np.array([np.sqrt(sumsq_ref(X[:, j])) for j in range(k)])
    assert np.array_equal(bits(got[:k]), bits(ref))
    assert np.all(got[k:] == -1.0)
    assert np.array_equal(bits(Xd.cpu().numpy()), bits(X))
    lib.call("mlamg_remove_mean_mv", lib.ptr(Xd), ld, n, k, s)
    got = Xd.cpu().numpy()
    for j in range(k):
        assert np.array_equal(bits(got[:, j]), bits(remove_mean_ref(X[:, j]))), j
    assert np.array_equal(bits(got[:, k:]), bits(X[:, k:]))  # the padding columns: untouched


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 256, 257, 7169 * 256 + 1))
def test_residual_norm_is_the_stated_order(torch_cuda, lib, n):
    """mlamg_residual's fused norm with no format set. The row-block rule (csr_finalize): a block
    is consecutive rows while it has <= 256 rows and <= 2048 nonzeros, so a diagonal matrix has
    blocks of exactly 256 rows; thread t of block b owns row 256 b + t and adds r^2 once to its
    +0.0; block b's total is partial b, and 1024 threads sum the partials. At the last size
    (7170 partials) thread 0 of that workgroup takes strided_sum's 8-way unrolled loop."""
    import mlamg.sparse
    torch = torch_cuda
    rs = np.random.RandomState(n % 1000)
    d = 1.0 + rs.random_sample(n)
    x, b = ill_scaled(n, 11), ill_scaled(n, 12)
    Ad = mlamg.sparse.DeviceCSR.from_scipy(sp.diags(d).tocsr())
    r = torch.empty(n, dtype=torch.float64, device="cuda")
    nrm = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    bd, xd = dev(torch, b), dev(torch, x)
    lib.call("mlamg_residual", Ad.handle, lib.ptr(bd), lib.ptr(xd), lib.ptr(r), lib.ptr(nrm),
             lib.stream_ptr())
    rh = r.cpu().numpy()
    assert np.array_equal(rh, b - d * x)
    nb = -(-n // 256)
    ref = np.sqrt(partials_total(block_totals(thread_sums(rh * rh, nb, 256)), 1024))
    assert np.array_equal(bits(nrm.cpu().numpy()), bits([ref]))
