"""GPU: the wide GNN kernels of csrc/gnn_wide.hip through the C-ABI, each on its own.

mlamg_gnn_linear_wide computes every output as one k-ordered fmaf chain from +0.0 (the f32-input
matrix cores round once per product), so it is held to VALUE EQUALITY, not a tolerance: with
mlamg_gnn_linear wherever both accept the shape, and with a host std::fmaf model
(tests/host/linear_model_driver.cpp) beyond. Equality is np.array_equal on values: zero padding can
turn a -0.0 sum into +0.0. mlamg_gnn_propagate_wide is bitwise mlamg_gnn_propagate column by
column. layer_norm, edge_in and standardize_abs are compared with float64 numpy references under
the rule of tests/test_gpu_gnn_kernels.py: err_dev <= max(4 err_ref32, 4 * 2^-24 * scale), err_ref32
the error of a torch fp32 restatement, scale = max|ref64|. Outputs are NaN before every call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def host_model(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("linear_model") / "driver")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "host", "linear_model_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _rs(*key):
    from oracle import gnn_kernel_cases as gc
    return gc._seed(*key)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _nan(torch, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _up(torch, a):
    """Upload; the caller keeps the tensor in a variable until its kernel has been launched (a
    temporary's block would be handed to the next upload and overwritten before the launch)."""
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _refused(torch, name, *args):
    from mlamg import _lib
    conv = [_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    assert getattr(_lib.lib, name)(*conv, _lib.stream_ptr()) == _lib.MLAMG_EINVAL, name
    torch.cuda.synchronize()


def _all_nan(t):
    return bool(t.isnan().all().item())


def _judge(label, dev, ref64, ref32):
    from oracle import gnn_kernel_cases as gc
    ref64 = np.asarray(ref64, dtype=np.float64)
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    err32 = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max())
    err = float(np.abs(dev.astype(np.float64) - ref64).max())
    tol = gc.tolerance(err32, scale)
    s = max(scale, 1e-300)
    print(f"[gnn-wide] {label}: err_dev/scale {err / s:.3e} err_ref32/scale {err32 / s:.3e} "
          f"ratio {err / max(err32, gc.F32_EPS * scale, 1e-300):.3f}")
    assert err <= tol, (label, err, tol)  # NaN in dev fails


# -------------------------------------------------------------------------------------- linear
def _linear_case(M, K, N, has_b, act, beta, rc, key):
    rs = _rs(M, K, N, key)
    return dict(M=M, K=K, N=N, act=act, beta=beta, rc=rc,
                X=_f(rs.randn(M, K)), W=_f(rs.randn(N, K) / np.sqrt(K)),
                b=_f(rs.randn(N)) if has_b else None,
                R=_f(rs.randn(M, rc)) if rc else None,
                Y0=_f(rs.randn(M, N)) if beta != 0.0 else None)


def _run_linear(torch, name, c):
    from mlamg._lib import call, ptr, stream_ptr
    Y = _up(torch, c["Y0"]) if c["beta"] != 0.0 else _nan(torch, c["M"], c["N"])
    X, W, b, R = (_up(torch, c[k]) for k in ("X", "W", "b", "R"))
    call(name, ptr(X), c["M"], c["K"], ptr(W), ptr(b), c["N"], c["act"], c["beta"], ptr(R),
         c["rc"], ptr(Y), stream_ptr())
    return Y.cpu().numpy()


def _combos(N):
    """(bias, act, beta, rc): with and without bias, act 0/1, beta 0/1, rc in {0, 1, N}."""
    return [(hb, act, beta, rc) for hb in (0, 1) for act in (0, 1) for beta in (0.0, 1.0)
            for rc in sorted({0, 1, N})]


@pytest.mark.parametrize("shape", ((1, 1, 1), (5, 7, 3), (257, 160, 64), (33, 3, 64)),
                         ids=lambda s: "x".join(map(str, s)))
def test_linear_wide_equals_narrow_kernel(torch_cuda, shape):
    M, K, N = shape
    for key, (hb, act, beta, rc) in enumerate(_combos(N)):
        c = _linear_case(M, K, N, hb, act, beta, rc, key)
        wide = _run_linear(torch_cuda, "mlamg_gnn_linear_wide", c)
        narrow = _run_linear(torch_cuda, "mlamg_gnn_linear", c)
        assert np.isfinite(narrow).all()
        assert np.array_equal(wide, narrow), (shape, hb, act, beta, rc,
                                              int((wide != narrow).sum()))


@pytest.mark.parametrize("shape", ((1, 161, 65), (33, 513, 255), (257, 1024, 256), (64, 2, 256),
                                   (130, 35, 129), (128, 64, 128), (127, 64, 128)),
                         ids=lambda s: "x".join(map(str, s)))
def test_linear_wide_equals_host_fmaf_model(torch_cuda, host_model, tmp_path, shape):
    """Odd K against the x2 MFMA step, M and N off the 64 x 64 tile (by one, by one less, not at
    all), the limits themselves."""
    M, K, N = shape
    for key, (hb, act, beta, rc) in enumerate(((0, 0, 0.0, 0), (1, 1, 1.0, N), (1, 0, 1.0, 1))):
        c = _linear_case(M, K, N, hb, act, beta, rc, 100 + key)
        fin, fout = tmp_path / f"in{key}.bin", tmp_path / f"out{key}.bin"
        with open(fin, "wb") as f:
            np.asarray([M, K, N, act, hb, rc], dtype=np.int64).tofile(f)
            np.asarray([beta], dtype=np.float32).tofile(f)
            for a in (c["X"], c["W"], c["b"], c["R"], c["Y0"]):
                if a is not None:
                    a.tofile(f)
        r = subprocess.run([host_model, str(fin), str(fout)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        want = np.fromfile(fout, dtype=np.float32).reshape(M, N)
        got = _run_linear(torch_cuda, "mlamg_gnn_linear_wide", c)
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), (shape, key, int((got != want).sum()))


def test_linear_wide_refusals_and_empty(torch_cuda):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    for K, N, beta, rc in ((0, 4, 0.0, 0), (1025, 4, 0.0, 0), (4, 257, 0.0, 0), (4, 4, 0.5, 0),
                           (4, 4, 0.0, 2)):
        Y = _nan(torch, 4, N)
        _refused(torch, "mlamg_gnn_linear_wide", z(4, max(K, 1)), 4, K, z(N, max(K, 1)), None, N,
                 0, beta, z(4, rc) if rc else None, rc, Y)
        assert _all_nan(Y), (K, N, beta, rc)
    Y = _nan(torch, 1, 4)
    call("mlamg_gnn_linear_wide", None, 0, 4, ptr(z(4, 4)), None, 4, 0, 0.0, None, 0, ptr(Y),
         stream_ptr())  # M == 0: returns at once
    torch.cuda.synchronize()
    assert _all_nan(Y)


# ----------------------------------------------------------------------------------- propagate
def _propagate(torch, name, g, w, X):
    from mlamg._lib import call, ptr, stream_ptr
    F = X.shape[1]
    Y = _nan(torch, g.n, F)
    tptr, teid, src, wd, Xd = (_up(torch, a) for a in (g.tptr, g.teid, g.src, w, X))
    call(name, ptr(tptr), ptr(teid), ptr(src), ptr(wd), ptr(Xd), g.n, F, ptr(Y), stream_ptr())
    return Y.cpu().numpy()


@pytest.mark.parametrize("gname", ("dir7", "ragged301", "empty5"))
def test_propagate_wide_columns_are_the_narrow_kernel(torch_cuda, gname):
    from oracle import gnn_kernel_cases as gc
    g = gc.GRAPHS[gname]()
    for F in (1, 65, 256):
        X = _f(_rs(g.n, F, 7).randn(g.n, F))
        wide = _propagate(torch_cuda, "mlamg_gnn_propagate_wide", g, g.w, X)
        assert np.isfinite(wide).all()
        for f in sorted({0, F // 2, 63 % F, 64 % F, F - 1}):
            col = _propagate(torch_cuda, "mlamg_gnn_propagate", g, g.w, _f(X[:, f:f + 1]))
            assert np.array_equal(wide[:, f].view(np.uint32), col[:, 0].view(np.uint32)), (F, f)
        if F <= 64:
            narrow = _propagate(torch_cuda, "mlamg_gnn_propagate", g, g.w, X)
            assert np.array_equal(wide.view(np.uint32), narrow.view(np.uint32))


def test_propagate_wide_refuses_wider_rows(torch_cuda):
    from oracle import gnn_kernel_cases as gc
    torch, g = torch_cuda, gc.dir7()
    Y = _nan(torch, g.n, 257)
    X = torch.zeros((g.n, 257), dtype=torch.float32, device="cuda")
    _refused(torch, "mlamg_gnn_propagate_wide", _up(torch, g.tptr), _up(torch, g.teid),
             _up(torch, g.src), _up(torch, g.w), X, g.n, 257, Y)
    assert _all_nan(Y)


# ---------------------------------------------------------------------------------- layer_norm
def _ln(x, w, b, eps):
    """LayerNorm in x's dtype (numpy float64 or torch float32 via the caller)."""
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * w + b


def _ln32(torch, x, w, b, eps):
    t = torch.as_tensor(x)
    return torch.nn.functional.layer_norm(t, (t.shape[1],), torch.as_tensor(w),
                                          torch.as_tensor(b), eps).numpy()


@pytest.mark.parametrize("rows", (1, 301))
@pytest.mark.parametrize("F", (1, 16, 255, 256))
def test_layer_norm(torch_cuda, rows, F):
    """Affine or none, residual or none, relu or none; row means several deviations off zero.
    At F = 1 every row is constant: the normalised value is exactly 0 and the output the bias."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    rs = _rs(rows, F, 3)
    X = _f(rs.randn(rows, F) * rs.uniform(0.5, 3.0, (rows, 1)) + rs.randn(rows, 1) * 4.0)
    w, b, R = _f(1.0 + 0.3 * rs.randn(F)), _f(rs.randn(F)), _f(rs.randn(rows, F))
    Xd, wd, bd, Rd = (_up(torch, a) for a in (X, w, b, R))
    for affine, res, act in ((1, 1, 1), (1, 0, 0), (0, 0, 0), (0, 1, 0)):
        Y = _nan(torch, rows, F)
        call("mlamg_gnn_layer_norm", ptr(Xd), rows, F, ptr(wd) if affine else None,
             ptr(bd) if affine else None, EPS, ptr(Rd) if res else None, act, ptr(Y),
             stream_ptr())
        dev = Y.cpu().numpy()
        ww, bb = (w, b) if affine else (np.ones(F, np.float32), np.zeros(F, np.float32))
        r64 = _ln(X.astype(np.float64), ww.astype(np.float64), bb.astype(np.float64), EPS)
        r32 = _ln32(torch, X, ww, bb, EPS)
        if res:
            r64, r32 = r64 + R, r32 + R
        if act:
            r64, r32 = np.maximum(r64, 0), np.maximum(r32, 0)
        if F == 1:
            want = np.broadcast_to(bb[None, :], (rows, 1)) + (R if res else np.float32(0))
            assert np.array_equal(dev, np.maximum(want, 0) if act else want)
        _judge(f"layer_norm {rows}x{F} affine{affine} res{res} act{act}", dev, r64, r32)


def test_layer_norm_refusal_and_empty(torch_cuda):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    Y = _nan(torch, 3, 257)
    _refused(torch, "mlamg_gnn_layer_norm", torch.zeros_like(Y), 3, 257, None, None, EPS, None, 0,
             Y)
    assert _all_nan(Y)
    call("mlamg_gnn_layer_norm", None, 0, 8, None, None, EPS, None, 0, None, stream_ptr())


# ------------------------------------------------------------------------------------- edge_in
@pytest.mark.parametrize("H", (1, 65, 256))
def test_edge_in(torch_cuda, H):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    from oracle import gnn_kernel_cases as gc
    g = gc.ragged301()
    rs = _rs(g.n, H, 11)
    U, V = _f(rs.randn(g.n, H)), _f(rs.randn(g.n, H))
    ea, w, b = _f(g.w), _f(rs.randn(H)), _f(rs.randn(H))
    gam, bet = _f(1.0 + 0.3 * rs.randn(H)), _f(rs.randn(H))
    out = _nan(torch, g.E, H)
    d = [_up(torch, a) for a in (g.src, g.tgt, U, V, ea, w, b, gam, bet)]
    call("mlamg_gnn_edge_in", *(ptr(a) for a in d[:5]), g.E, H, *(ptr(a) for a in d[5:]), EPS,
         ptr(out), stream_ptr())

    def pre(dt):
        return (U.astype(dt)[g.src] + V.astype(dt)[g.tgt] + ea.astype(dt)[:, None] * w.astype(dt)
                + b.astype(dt))

    r64 = np.maximum(_ln(pre(np.float64), gam.astype(np.float64), bet.astype(np.float64), EPS), 0)
    r32 = np.maximum(_ln32(torch, pre(np.float32), gam, bet, EPS), 0)
    _judge(f"edge_in H{H}", out.cpu().numpy(), r64, r32)


def test_edge_in_refusal_and_empty(torch_cuda):
    torch = torch_cuda
    from mlamg._lib import call, stream_ptr
    from oracle import gnn_kernel_cases as gc
    g = gc.dir7()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    out = _nan(torch, g.E, 257)
    _refused(torch, "mlamg_gnn_edge_in", _up(torch, g.src), _up(torch, g.tgt), z(g.n, 257),
             z(g.n, 257), z(g.E), g.E, 257, z(257), z(257), z(257), z(257), EPS, out)
    assert _all_nan(out)
    call("mlamg_gnn_edge_in", None, None, None, None, None, 0, 8, None, None, None, None, EPS,
         None, stream_ptr())  # E == 0


# ----------------------------------------------------------------------------- standardize_abs
@pytest.mark.parametrize("E", (2, 301, 200001))
def test_standardize_abs(torch_cuda, E):
    """E = 200001 spreads the sums over many workgroups (the fixed grid of reduce.hpp)."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    v = _f(_rs(E, 5).randn(E) * 0.7 + 3.0)
    out = _nan(torch, E)
    vd = _up(torch, v)
    call("mlamg_gnn_standardize_abs", ptr(vd), E, ptr(out), stream_ptr())
    v64 = v.astype(np.float64)
    r64 = np.abs((v64 - v64.mean()) / v64.std(ddof=1))
    t = torch.as_tensor(v)
    r32 = torch.abs((t - t.mean()) / t.std()).numpy()
    _judge(f"standardize_abs E{E}", out.cpu().numpy(), r64, r32)


def test_standardize_abs_refuses_one_value(torch_cuda):
    torch = torch_cuda
    out = _nan(torch, 1)
    _refused(torch, "mlamg_gnn_standardize_abs", torch.ones(1, device="cuda"), 1, out)
    assert _all_nan(out)
