"""One handle walked through every storage format, forwards and backwards: each conversion
goes through the single set-aside / build / drop path of mlamg_csr_set_format (csrc/formats.hip),
which the other tests exercise on fresh handles or in one direction only."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

FORWARD = (("csr_stream", 0), ("sell", 0), ("sell_dict", 0), ("sorted", 0), ("sorted", 1),
           ("sorted", 2), ("long", 0), ("rowpat", 0), ("vector", 64), ("auto_exact", 0),
           ("csr_stream", 0))
WALK = FORWARD + FORWARD[::-1]

# Conversions refused with MLAMG_EUNSUPPORTED, and what auto_exact settles on: recorded from this
# walk on the commit before set_format got its single drop path. sell_dict and rowpat need few
# distinct values / row-pair patterns; sorted value codes (2) are refused where the one-byte
# dictionary applies (Poisson) and where a block's values are mostly distinct (random).
REFUSED = {"poisson": {("sorted", 2)},
           "random": {("sell_dict", 0), ("sorted", 2), ("rowpat", 0)}}
AUTO_EXACT = {"poisson": "sell", "random": "sell"}


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


def dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


def matrices(ml):
    """529 rows (23 x 23 grid): an odd row count (a single last row pair), three CSR-stream row
    blocks, nine SELL slices; once with the stencil's two values, once with random ones."""
    P = ml.problems.poisson_2d_5pt(23).tocsr()
    assert P.shape == (529, 529)
    R = sp.csr_matrix((P.data * np.random.RandomState(3).uniform(0.5, 1.5, P.nnz), P.indices,
                       P.indptr), shape=P.shape)
    return {"poisson": P, "random": R}


class Probe:
    """The three results the walk compares, on one handle and fixed vectors."""

    def __init__(self, ml, torch, A):
        from mlamg._lib import call, ptr, stream_ptr
        self.call, self.ptr, self.stream_ptr, self.torch = call, ptr, stream_ptr, torch
        rs = np.random.RandomState(7)
        n = A.shape[0]
        self.x, self.b = rs.randn(n), rs.randn(n)
        self.Ad = ml.sparse.DeviceCSR.from_scipy(A)
        self.dinv = self.Ad.diag_inv(2.0 / 3.0)
        self.xd, self.bd = dev(torch, self.x), dev(torch, self.b)
        d = self.dinv.cpu().numpy()
        Ax = A @ self.x
        self.ref = (Ax, self.x + d * (self.b - Ax), self.b - Ax)  # scipy's bits

    def jacobi(self):
        xs, t = self.xd.clone(), self.torch.empty_like(self.xd)
        self.call("mlamg_jacobi", self.Ad.handle, self.ptr(self.dinv), self.ptr(self.bd),
                  self.ptr(xs), self.ptr(t), 1, self.stream_ptr())
        return xs.cpu().numpy()

    def results(self):
        """(A @ x, one Jacobi sweep, residual, residual norm)"""
        torch = self.torch
        r = torch.empty_like(self.bd)
        nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.call("mlamg_residual", self.Ad.handle, self.ptr(self.bd), self.ptr(self.xd),
                  self.ptr(r), self.ptr(nrm), self.stream_ptr())
        return (self.Ad.matvec(self.xd).cpu().numpy(), self.jacobi(), r.cpu().numpy(),
                nrm.item())


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def walk(p):
    """Yield (requested, refused, format before, results before, format after, results after)
    for every step of WALK; a refusal is an MlamgError with MLAMG_EUNSUPPORTED."""
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    for req in WALK:
        f0, r0 = p.Ad.get_format(), p.results()
        refused = False
        try:
            p.Ad.set_format(*req)
        except MlamgError as e:
            assert e.code == MLAMG_EUNSUPPORTED, e
            refused = True
        yield req, refused, f0, r0, p.Ad.get_format(), p.results()


@pytest.mark.parametrize("name", ("poisson", "random"))
def test_format_walk_forwards_and_backwards(ml, torch_cuda, name):
    A = matrices(ml)[name]
    p = Probe(ml, torch_cuda, A)
    nref = np.linalg.norm(p.ref[2])
    vector_results = None
    for req, refused, f0, r0, f1, r1 in walk(p):
        print(name, req, "refused" if refused else "ok", f0, "->", f1, "norm", repr(r1[3]))
        assert refused == (req in REFUSED[name]), (req, refused)
        if refused:  # the handle is exactly as it was
            assert f1 == f0 and same(r1, r0), (req, f0, f1)
        elif req[0] == "auto_exact":
            assert f1[0] == AUTO_EXACT[name]
        else:
            assert f1[0] == req[0], (req, f1)
        if f1[0] == "vector":  # its own summation order: the same bits on every visit
            vector_results = vector_results or r1
            assert same(r1, vector_results)
            assert np.allclose(r1[0], p.ref[0], rtol=1e-11, atol=1e-11)
        else:  # exact-order formats: scipy's bits
            assert same(r1[:3], p.ref), (req, f1)
            assert abs(r1[3] - nref) <= 1e-13 * nref, (req, f1, r1[3], nref)


def test_attached_weights_across_formats(ml, torch_cuda):
    """attach_dinv on a rowpat handle, then sell, then rowpat again: the Jacobi sweep given the
    same dinv tensor is scipy's bits at each point, and leaving rowpat detaches."""
    p = Probe(ml, torch_cuda, matrices(ml)["poisson"])
    p.Ad.set_format("rowpat")
    assert p.Ad.attach_dinv(p.dinv)
    assert np.array_equal(p.jacobi(), p.ref[1])
    p.Ad.set_format("sell")
    assert p.Ad.get_format()[0] == "sell"
    assert np.array_equal(p.jacobi(), p.ref[1])
    assert not p.Ad.attach_dinv(p.dinv)  # not rowpat: nothing attached
    p.Ad.set_format("rowpat")
    assert p.Ad.get_format()[0] == "rowpat"
    assert np.array_equal(p.jacobi(), p.ref[1])
