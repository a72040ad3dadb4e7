"""GPU: the segmented per-column norm and mean removal (mlamg_norm2_seg_mv,
mlamg_remove_mean_seg_mv; csrc/seg_mv.hip). Every segment's result is bitwise
mlamg_norm2_mv / mlamg_remove_mean_mv on a copy of that segment's rows alone.

One multivector with segments of 1, 255, 256, 257 and 1,000 rows (below, at and above one row
block) and one of 262,400 rows: 1,025 row blocks, past the 1,024-block cap of the norm and the
512-block grid of the mean, so the strided walk of both takes more than one step there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEGMENTS = (1, 255, 256, 257, 1000, 262400)
#        k  extra leading dimension
CASES = ((1, 0), (8, 0), (9, 3), (64, 0))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.mark.parametrize("k,pad", CASES)
def test_segments_are_bitwise_the_single_kernels(torch_cuda, k, pad):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    off = np.concatenate([[0], np.cumsum(SEGMENTS)]).astype(np.int64)
    n, nb, max_len = int(off[-1]), len(SEGMENTS), max(SEGMENTS)
    g = torch.Generator(device="cuda").manual_seed(100 + k)
    # columns of very different means and scales, so a wrong divisor or partition shows
    full = torch.randn((n, k + pad), generator=g, dtype=torch.float64, device="cuda")
    full = full * torch.logspace(-3, 3, k + pad, dtype=torch.float64, device="cuda") + 0.5
    X = full[:, :k]
    ld = k + pad
    off_d = torch.as_tensor(off).cuda()
    s = stream_ptr()

    def single(seg):
        a, b = int(off[seg]), int(off[seg + 1])
        Y = X[a:b].clone().contiguous()
        nrm = torch.empty(k, dtype=torch.float64, device="cuda")
        call("mlamg_norm2_mv", ptr(Y), k, b - a, k, ptr(nrm), s)
        call("mlamg_remove_mean_mv", ptr(Y), k, b - a, k, s)
        return nrm.cpu().numpy(), Y.cpu().numpy()

    want = [single(i) for i in range(nb)]
    norms = torch.full((nb, k), -1.0, dtype=torch.float64, device="cuda")
    call("mlamg_norm2_seg_mv", ptr(X), ld, k, ptr(off_d), nb, max_len, ptr(norms), s)
    before = full.clone()
    call("mlamg_remove_mean_seg_mv", ptr(X), ld, k, ptr(off_d), nb, max_len, s)
    norms, got = norms.cpu().numpy(), X.cpu().numpy()
    for i in range(nb):
        a, b = int(off[i]), int(off[i + 1])
        assert np.array_equal(norms[i], want[i][0]), (i, SEGMENTS[i])
        assert np.array_equal(got[a:b], want[i][1]), (i, SEGMENTS[i])
    # the single kernels did something to compare against, and the padding columns are untouched
    assert np.all(norms > 0) and not np.array_equal(got, before[:, :k].cpu().numpy())
    if pad:
        assert torch.equal(full[:, k:], before[:, k:])
