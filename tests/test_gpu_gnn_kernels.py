"""GPU: every GNN inference kernel of csrc/gnn.hip (mlamg_gnn_linear, _gcn_norm, _propagate,
_instance_norm, _nnconv, _edge_mlp, _topk) called through the C-ABI on its own and compared with
a float64 numpy reference of the same operation (oracle/gnn_kernels_ref.py), at ragged shapes, on
directed graphs, at the size limits of include/mlamg.h and past the 4 x 2^20 items a capped grid
would cover. Cases, references and the tolerance rule live in oracle/gnn_kernel_cases.py and are
validated on the CPU by tests/test_gnn_kernels_ref_host.py.

Tolerance, per floating-point output tensor: scale = max|ref64|, err_ref32 = the error of the
torch fp32 restatement of the same case, and
    err_dev = max|dev - ref64| <= max(4 err_ref32, 4 * 2^-24 * scale)
with the same factor for every case. Every output is filled with NaN before the call, so an entry
the kernel does not write fails the comparison. Every test prints err_dev / scale,
err_ref32 / scale and their ratio per case (pytest -s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _cases(name):
    from oracle import gnn_kernel_cases as gc
    return getattr(gc, name + "_cases")()


def _ids(name):
    return [c["id"] for c in _cases(name)]


class _Dev:
    """Uploads a case's arrays (a numpy view shares its base's buffer) and calls the C-ABI."""

    def __init__(self, torch):
        self.torch = torch
        self.memo = {}

    def up(self, a):
        if a is None:
            return None
        base = a if a.base is None else a.base
        assert a.flags.c_contiguous and base.flags.c_contiguous
        if id(base) not in self.memo:
            self.memo[id(base)] = self.torch.as_tensor(base).reshape(-1).cuda()
        off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0])
        off //= a.itemsize
        return self.memo[id(base)][off:off + a.size].reshape(a.shape)

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), dtype=self.torch.float32, device="cuda")

    def run(self, c):
        """The case on the device: {output name: numpy array} (+ "msg": the NNConv scratch)."""
        from mlamg._lib import call, ptr, stream_ptr
        k, g, up = c["kernel"], c.get("graph"), self.up
        if k == "linear":
            Y = up(c["Y0"]).clone() if c["beta"] != 0.0 else self.nan(c["M"], c["N"])
            R = up(c["R"])
            call("mlamg_gnn_linear", ptr(up(c["X"])), c["M"], c["K"], ptr(up(c["W"])),
                 ptr(up(c["b"])), c["N"], c["act"], c["beta"], ptr(R),
                 0 if R is None else R.shape[1], ptr(Y), stream_ptr())
            out = {"Y": Y}
        elif k == "gcn_norm":
            dis, wn = self.nan(g.n), self.nan(g.E)
            call("mlamg_gnn_gcn_norm", ptr(up(g.tptr)), ptr(up(g.teid)), ptr(up(g.src)),
                 ptr(up(g.tgt)), ptr(up(g.w)), g.n, g.E, ptr(dis), ptr(wn), stream_ptr())
            out = {"dis": dis, "wn": wn}
        elif k == "propagate":
            Y = self.nan(g.n, c["F"])
            call("mlamg_gnn_propagate", ptr(up(g.tptr)), ptr(up(g.teid)), ptr(up(g.src)),
                 ptr(up(c["w"])), ptr(up(c["X"])), g.n, c["F"], ptr(Y), stream_ptr())
            out = {"Y": Y}
        elif k == "instance_norm":
            Y = self.nan(c["n"], c["F"])
            call("mlamg_gnn_instance_norm", ptr(up(c["X"])), c["n"], c["F"], c["eps"], ptr(Y),
                 stream_ptr())
            out = {"Y": Y}
        elif k == "nnconv":
            R = up(c["R"])
            msg, Y = self.nan(max(g.E, 1), c["Fout"]), self.nan(g.n, c["Fout"])
            call("mlamg_gnn_nnconv", ptr(up(g.tptr)), ptr(up(g.teid)), ptr(up(g.src)),
                 ptr(up(c["ea"])), g.E, c["fe"], ptr(up(c["L1"])), ptr(up(c["c1"])),
                 ptr(up(c["L2"])), ptr(up(c["c2"])), ptr(up(c["L3"])), ptr(up(c["c3"])),
                 ptr(up(c["X"])), g.n, c["Fin"], c["Fout"], ptr(up(c["root"])),
                 ptr(up(c["bias"])), c["act"], ptr(R), 0 if R is None else R.shape[1], ptr(msg),
                 ptr(Y), stream_ptr())
            out = {"Y": Y, "msg": msg}
        elif k == "edge_mlp":
            R = up(c["R"])
            o = self.nan(max(g.E, 1), c["C"])
            call("mlamg_gnn_edge_mlp", ptr(up(g.src)), ptr(up(g.tgt)), ptr(up(c["X"])), c["F"],
                 ptr(up(c["ea"])), c["fe"], g.E, ptr(up(c["W1"])), ptr(up(c["b1"])), c["H"],
                 ptr(up(c["g"])), ptr(up(c["beta"])), ptr(up(c["W2"])), ptr(up(c["b2"])),
                 c["C"], c["act"], ptr(R), 0 if R is None else R.shape[1], ptr(o), stream_ptr())
            out = {"out": o[:g.E] if g.E else o}
        else:
            raise KeyError(k)
        return {name: v.cpu().numpy() for name, v in out.items()}


def _judge(c, dev, yard=None):
    """Print the figures of every tensor of the case, then assert the rule on each."""
    from oracle import gnn_kernel_cases as gc
    rows = gc.judge(c, {k: v for k, v in dev.items() if k != "msg"}, yard)
    for label, err, err32, scale, tol, ok in rows:
        s = max(scale, 1e-300)
        ratio = err / max(err32, gc.F32_EPS * scale, 1e-300)
        print(f"[gnn-kernel] {c['kernel']} {c['id']} {label}: err_dev/scale {err / s:.3e} "
              f"err_ref32/scale {err32 / s:.3e} ratio {ratio:.3f}")
    for label, err, err32, scale, tol, ok in rows:
        assert ok, (c["kernel"], c["id"], label, err, tol)
    return rows


def _refused(torch, name, *args):
    """The entry point returns MLAMG_EINVAL for these arguments."""
    from mlamg import _lib
    conv = [_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    assert getattr(_lib.lib, name)(*conv, _lib.stream_ptr()) == _lib.MLAMG_EINVAL, name
    torch.cuda.synchronize()


def _all_nan(t):
    return bool(t.isnan().all().item())


# -------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("cid", _ids("linear"))
def test_linear(torch_cuda, cid):
    """N not a power of two (idle lanes of a row), K = 1 and K = 160, M = 0, bias or none, relu
    or none, beta = 1 on a random Y (beta = 0 on a NaN one: Y must not be read), residual none /
    one column / N columns."""
    c = next(c for c in _cases("linear") if c["id"] == cid)
    _judge(c, _Dev(torch_cuda).run(c))


def test_linear_refusals(torch_cuda):
    torch = torch_cuda
    d = _Dev(torch)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    for K, N, rc in ((161, 4, 0), (4, 65, 0), (4, 4, 2), (4, 4, 3)):
        Y = d.nan(4, N)
        _refused(torch, "mlamg_gnn_linear", z(4, K), 4, K, z(N, K), None, N, 0, 0.0,
                 z(4, max(rc, 1)) if rc else None, rc, Y)
        assert _all_nan(Y), (K, N, rc)


# ------------------------------------------------------------------------ gcn_norm / propagate
@pytest.mark.parametrize("cid", _ids("gcn_norm"))
def test_gcn_norm(torch_cuda, cid):
    """Directed graphs (the host test shows that reversed edges would be > 100 tolerances off), a
    graph without edges; a node without incoming edges has dis == 0 exactly."""
    c = next(c for c in _cases("gcn_norm") if c["id"] == cid)
    dev = _Dev(torch_cuda).run(c)
    _judge(c, dev)
    g = c["graph"]
    lone = np.bincount(g.tgt, minlength=g.n) == 0
    assert lone.any() and np.all(dev["dis"][lone] == 0.0)
    assert not np.signbit(dev["dis"][lone]).any()


@pytest.mark.parametrize("cid", _ids("propagate"))
def test_propagate(torch_cuda, cid):
    c = next(c for c in _cases("propagate") if c["id"] == cid)
    dev = _Dev(torch_cuda).run(c)
    _judge(c, dev)
    g = c["graph"]
    assert np.all(dev["Y"][np.bincount(g.tgt, minlength=g.n) == 0] == 0.0)


def test_propagate_refuses_wide_features(torch_cuda):
    from oracle import gnn_kernel_cases as gc
    d, g = _Dev(torch_cuda), gc.dir7()
    Y = d.nan(g.n, 65)
    X = torch_cuda.zeros((g.n, 65), dtype=torch_cuda.float32, device="cuda")
    _refused(torch_cuda, "mlamg_gnn_propagate", d.up(g.tptr), d.up(g.teid), d.up(g.src),
             d.up(g.w), X, g.n, 65, Y)
    assert _all_nan(Y)


# ------------------------------------------------------------------------------- instance_norm
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 1000))
def test_instance_norm(torch_cuda, n):
    """n below, at and across the block's 256 threads, F up to 130 blocks; channel means up to
    9.5 standard deviations off zero; an exactly constant channel (x = 1/n, and every channel at
    n = 1) is compared with 0 at scale |c| / sqrt(eps)."""
    d = _Dev(torch_cuda)
    mine = [c for c in _cases("instance_norm") if c["n"] == n]
    assert len(mine) == 4
    for c in mine:
        dev = d.run(c)
        _judge(c, dev)
        assert np.all(np.isfinite(dev["Y"]))


# -------------------------------------------------------------------------------------- nnconv
@pytest.mark.parametrize("cid", _ids("nnconv"))
def test_nnconv(torch_cuda, cid):
    """Fout below 16 (idle waves), no multiple of 16 (a partial output block), E no multiple of
    64 (dead lanes in the last tile), Fin = 1 and 64; relu or none; residual none / one column /
    Fout columns. Without edges the output is act(root + bias) (+ R) and the scratch stays
    untouched."""
    c = next(c for c in _cases("nnconv") if c["id"] == cid)
    dev = _Dev(torch_cuda).run(c)
    _judge(c, dev)
    if c["graph"].E == 0:
        assert np.isnan(dev["msg"]).all()
    else:
        assert np.isfinite(dev["msg"]).all()


def test_nnconv_refuses_wide_output(torch_cuda):
    torch = torch_cuda
    from oracle import gnn_kernel_cases as gc
    d, g = _Dev(torch), gc.dir7()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    Y, msg = d.nan(g.n, 65), d.nan(g.E, 65)
    _refused(torch, "mlamg_gnn_nnconv", d.up(g.tptr), d.up(g.teid), d.up(g.src), z(g.E, 1), g.E,
             1, z(4, 1), z(4), z(16, 4), z(16), z(65, 16), z(65), z(g.n, 1), g.n, 1, 65,
             z(g.n, 65), z(65), 0, None, 0, msg, Y)
    assert _all_nan(Y) and _all_nan(msg)


# ------------------------------------------------------------------------------------ edge_mlp
@pytest.mark.parametrize("cid", _ids("edge_mlp"))
def test_edge_mlp(torch_cuda, cid):
    """H below 64 (masked LayerNorm sums), H = 1 (zero variance: the output is
    act(W2 beta_ln + b2), shown for the reference by the host test), C up to 4, 2F + fe up to
    160; relu or none; residual none / one column / C columns."""
    c = next(c for c in _cases("edge_mlp") if c["id"] == cid)
    _judge(c, _Dev(torch_cuda).run(c))


def test_edge_mlp_without_edges_and_refusals(torch_cuda):
    torch = torch_cuda
    from oracle import gnn_kernel_cases as gc
    d = _Dev(torch)
    c = dict(gc.edge_mlp_cases()[1], graph=gc.empty5())
    c["ea"], c["R"] = c["ea"][:0], None
    c["X"] = c["X"][:5].copy()
    assert _all_nan(torch.as_tensor(d.run(c)["out"]))  # E == 0: OK, nothing written
    g = gc.dir7()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    for F, fe, H, C in ((80, 1, 4, 1), (2, 1, 65, 1), (2, 1, 4, 5)):
        K = 2 * F + fe
        out = d.nan(g.E, C)
        _refused(torch, "mlamg_gnn_edge_mlp", d.up(g.src), d.up(g.tgt), z(g.n, F), F,
                 z(g.E, fe), fe, g.E, z(H, K), z(H), H, z(H), z(H), z(C, H), z(C), C, 0, None, 0,
                 out)
        assert _all_nan(out), (F, fe, H, C)


# ---------------------------------------------------------------------------------------- topk
@pytest.mark.parametrize("kind", ("random", "equal", "ties", "relu70", "signed_zero", "inf"))
def test_topk(torch_cuda, kind):
    """vec and idx bitwise the stable descending sort under IEEE comparison (ties, -0.0 == +0.0
    among them, to the smaller index), for n in {1, 6, 257, 5000} and k in {0, 1, n // 10, n}.
    NaN scores are left out: numpy's argsort and torch.sort leave their place unspecified, so
    the reference has no answer for them either."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    from oracle import gnn_kernels_ref as kref
    mine = [c for c in _cases("topk") if c["kind"] == kind]
    assert mine
    for c in mine:
        s, k = torch.as_tensor(c["scores"]).cuda(), c["k"]
        n = s.numel()
        vec = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        idx = torch.full((max(k, 1),), -1, dtype=torch.int32, device="cuda")
        call("mlamg_gnn_topk", ptr(s), n, k, ptr(vec), ptr(idx), stream_ptr())
        rvec, ridx = kref.topk(c["scores"], k)
        assert np.array_equal(idx.cpu().numpy()[:k], ridx), c["id"]
        assert np.array_equal(vec.cpu().numpy().view(np.uint32), rvec.view(np.uint32)), c["id"]
        if k == 0:
            assert idx.cpu().tolist() == [-1]
        call("mlamg_gnn_topk", ptr(s), n, k, ptr(vec), None, stream_ptr())  # idx is optional
        assert np.array_equal(vec.cpu().numpy(), rvec), c["id"]


def test_topk_refuses_k_above_n(torch_cuda):
    torch = torch_cuda
    s = torch.zeros(6, dtype=torch.float32, device="cuda")
    vec = torch.full((6,), float("nan"), dtype=torch.float32, device="cuda")
    idx = torch.full((7,), -1, dtype=torch.int32, device="cuda")
    _refused(torch, "mlamg_gnn_topk", s, 6, 7, vec, idx)
    assert _all_nan(vec) and idx.cpu().tolist() == [-1] * 7


# ------------------------------------------------------------------------------------ grid cap
@pytest.mark.parametrize("kernel", ("propagate", "nnconv", "edge_mlp"))
def test_launch_covers_more_than_4M_items(torch_cuda, kernel):
    """The wave-per-item kernels at T = 4 * 2^20 + 5 items and their narrowest widths: a grid
    capped at 2^20 blocks of 4 waves without a loop leaves items from 4 * 2^20 on unwritten
    (NaN here). propagate (F = 1) and nnconv (Fin = Fout = fe = 1: k_nnconv_aggr) on the directed
    ring of T nodes, edge_mlp (F = fe = 1, H = 2, C = 1) on T edges over 1,000 nodes. The whole
    output obeys the rule; the last 16 entries are asserted apart. About 100 MB on the device.
    (k_nnconv_msg, k_deg_isqrt, k_gcn_weight and the top-k kernels take 64 or 256 items per block
    and share the loop idiom; a test past their cap would need gigabytes.)"""
    from oracle import gnn_kernel_cases as gc
    c = gc.gridcap_case(kernel)
    dev = _Dev(torch_cuda).run(c)
    name = "out" if kernel == "edge_mlp" else "Y"
    got = dev[name].reshape(-1)
    assert got.shape == (gc.T_CAP,)
    missing = np.flatnonzero(~np.isfinite(got))
    assert missing.size == 0, (missing.size, int(missing[0]))
    yard = gc.yardsticks(c)
    _judge(c, dev, yard)
    ref, _, _, tol = yard[name]
    tail = np.abs(got[-16:].astype(np.float64) - ref.reshape(-1)[-16:])
    assert np.all(np.isfinite(got[-16:])) and tail.max() <= tol, (tail.max(), tol)
