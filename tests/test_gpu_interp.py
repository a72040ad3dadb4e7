"""GPU: mlamg.interp.InterpolationNetwork (the learned P of ns/model/ali_interp.py) and the
preconditioner options that use it, on the 12 x 12 grid with the reference's own C/F splitting at
theta 0.56 (50 coarse points, tests/golden/greedy_cf.npz) and seeded weights.

The yardstick is tests/interp_ref.py (validated on the CPU by tests/test_interp_host.py). Rule,
as in tests/test_gpu_gnn_kernels.py: err_dev = max|dev - ref64| <= max(4 err_ref32,
4 * 2^-24 * scale), scale = max|ref64|.
 - layer by layer: every device layer is fed the device's previous output; ref64 / ref32 are the
   restatement's layer on that same input in float64 / float32;
 - end to end on the edge values and on P: err_ref32 is the larger error of two float32
   evaluations of the whole restatement (natural order; features and edges reversed), so the bound
   reflects the spread of legitimate float32 orders; P's pattern, column order and unit rows on C
   are exact.
Every figure is printed (pytest -s)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import greedy_cases as gcases
import interp_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = 2.0 ** -24


class _Mat:
    def __init__(self, A):
        self.A = A.tocsr()

    def getValuesCSR(self):
        return self.A.indptr, self.A.indices, self.A.data


class _PC:
    def __init__(self, A, prefix=""):
        self.m = _Mat(A)
        self.prefix = prefix

    def getOperators(self):
        return self.m, self.m

    def getOptionsPrefix(self):
        return self.prefix


@pytest.fixture(scope="module")
def setup():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mlamg import interp
    gold = np.load(os.path.join(ROOT, "tests", "golden", "greedy_cf.npz"), allow_pickle=False)
    A = gcases.poisson_2d(12)
    C, F = gold["grid_12_C"], gold["grid_12_F"]
    assert len(C) == 50
    net = interp.InterpolationNetwork()
    sd = {k: v.clone() for k, v in interp_ref.seeded_state_dict(net.model, 2024).items()}
    net.cuda()
    g = net.graph_from_matrix(A, C, F)
    src, tgt = g.src.cpu().numpy(), g.tgt.cpu().numpy()
    ea = g.edge_attr.cpu().numpy()[:, 0]

    def ref(dtype, reverse=False):
        return interp_ref.Ref(sd, src, tgt, ea, dtype, reverse)

    # the whole restatement once: float64, and float32 in two orders
    x0 = g.x.cpu().numpy()
    e64 = ref(torch.float64).forward(x0)[1].numpy()
    e32 = [ref(torch.float32, rev).forward(x0)[1].numpy() for rev in (False, True)]
    return dict(torch=torch, A=A, C=C, F=F, net=net, sd=sd, g=g, ref=ref, e64=e64, e32=e32,
                src=src, tgt=tgt)


def _judge(label, dev, r64, r32s):
    r64 = np.asarray(r64, dtype=np.float64)
    scale = float(np.abs(r64).max())
    err32 = max(float(np.abs(np.asarray(r, dtype=np.float64) - r64).max()) for r in r32s)
    err = float(np.abs(np.asarray(dev, dtype=np.float64).reshape(r64.shape) - r64).max())
    tol = max(4.0 * err32, 4.0 * F32_EPS * scale)
    print(f"[interp] {label}: err_dev/scale {err / scale:.3e} err_ref32/scale "
          f"{err32 / scale:.3e} ratio {err / max(err32, F32_EPS * scale):.3f}")
    return label, err, tol


def test_layers_match_restatement(setup):
    s = setup
    torch, g, model = s["torch"], s["g"], s["net"].model
    r64, r32 = s["ref"](torch.float64), s["ref"](torch.float32)
    rows = []
    with torch.no_grad():
        x = g.x
        for i in range(model.n_blocks):
            xin = x.cpu().numpy()
            x = model.node_layer(i, g, x)
            rows.append(_judge(f"node block {i} ({x.shape[1]} ch)", x.cpu().numpy(),
                               r64.node_layer(i, xin).numpy(), [r32.node_layer(i, xin).numpy()]))
        assert x.shape == (g.n, 256)
        e = x
        for i in range(model.edge_model.n_blocks):
            ein = e.cpu().numpy()
            e = model.edge_model.layer(i, g, e)
            rows.append(_judge(f"edge block {i} ({e.shape[1]} ch)", e.cpu().numpy(),
                               r64.edge_layer(i, ein).numpy(), [r32.edge_layer(i, ein).numpy()]))
        assert e.shape == (g.E, 1)
        from mlamg import interp
        v = interp.standardize_abs(e)
        rows.append(_judge("standardize_abs", v.cpu().numpy(),
                           r64.standardize(e.cpu().numpy()).numpy(),
                           [r32.standardize(e.cpu().numpy()).numpy()]))
    assert len(rows) == 11 + 11 + 1
    for label, err, tol in rows:
        assert err <= tol, (label, err, tol)


def test_edge_values_and_P_end_to_end(setup):
    s = setup
    torch, g, net, A, C, F = s["torch"], s["g"], s["net"], s["A"], s["C"], s["F"]
    n = A.shape[0]
    vals = net.model.run(g).cpu().numpy()
    assert vals.shape == (g.E, 1) and np.all(vals >= 0)
    label, err, tol = _judge("edge values", vals, s["e64"], s["e32"])
    assert err <= tol, (label, err, tol)
    P = net.forward_mat(A, C, F)
    assert sp.isspmatrix_csr(P) and P.shape == (n, len(C)) and P.dtype == np.float64
    refs = [interp_ref.scipy_P(n, s["src"], s["tgt"], e, C) for e in [s["e64"]] + s["e32"]]
    for r in refs:
        r.sort_indices()
    # pattern, column order and the unit rows on C are exact
    assert np.array_equal(P.indptr, refs[0].indptr) and np.array_equal(P.indices, refs[0].indices)
    for col, c in enumerate(C):
        row = P.getrow(c)
        assert row.nnz == 1 and row.indices[0] == col and row.data[0] == 1.0
    is_c = np.zeros(n, dtype=bool)
    is_c[C] = True
    assert np.array_equal(np.diff(P.indptr)[~is_c],
                          np.asarray((A[:, C] != 0).sum(axis=1)).ravel()[~is_c])
    assert np.array_equal(P.data, P.data.astype(np.float32).astype(np.float64))  # fp32 values
    label, err, tol = _judge("P values", P.data, refs[0].data, [r.data for r in refs[1:]])
    assert err <= tol, (label, err, tol)
    # forward_mat is deterministic
    assert np.array_equal(net.forward_mat(A, C, F).data, P.data)


def test_too_few_edges_is_refused(setup):
    s = setup
    A = gcases.all_fine(7)
    with pytest.raises(ValueError, match="fewer than two edges"):
        s["net"].forward_mat(A, np.array([], dtype=np.int64), np.arange(7))


@pytest.fixture()
def options():
    import mlamg.preconditioner as pre
    pre._Options.store.clear()
    yield pre._Options.store
    pre._Options.store.clear()


def test_preconditioner_builds_the_learned_P(setup, options, tmp_path):
    s = setup
    torch, A, C, F = s["torch"], s["A"], s["C"], s["F"]
    import mlamg.preconditioner as pre
    from mlamg.greedy import greedy_coarsening
    path = str(tmp_path / "pnet.pt")
    torch.save(s["sd"], path)
    options.update({"mlamg_pnet_model": path, "mlamg_max_iter": 5})
    pc = _PC(A)
    M = pre.MLAMG()
    M.initialize(pc)
    assert M.coarsening_theta == 0.56 and M.pnet_model_fname == path
    _, F2, C2 = greedy_coarsening(A, 0.56)
    assert np.array_equal(C2, C) and np.array_equal(F2, F)
    want = s["net"].forward_mat(A, C, F)
    got = M.H.levels[0].P.to_scipy()
    assert got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, want.data)
    assert M.H.n_levels == 2
    n = A.shape[0]
    b = np.random.RandomState(1).randn(n)

    class Vec:
        def __init__(self, a):
            self.array_r = a
            self.out = None

        def setArray(self, v):
            self.out = np.array(v, copy=True)

    Y = Vec(None)
    np.random.seed(5)
    M.apply(pc, Vec(b), Y)
    assert Y.out.shape == (n,) and np.all(np.isfinite(Y.out))
    # the other theta of the option: another splitting, another P
    options.update({"mlamg_greedy_theta": 0.7})
    M2 = pre.MLAMG()
    M2.initialize(pc)
    assert M2.H.levels[0].P.shape == (n, 72)


def test_preconditioner_bad_model_path(setup, options, tmp_path):
    import mlamg.preconditioner as pre
    options.update({"mlamg_pnet_model": str(tmp_path / "missing.pt")})
    with pytest.raises(RuntimeError, match="Could not load PNet model"):
        pre.MLAMG().initialize(_PC(setup["A"]))
    bad = str(tmp_path / "bad.pt")
    setup["torch"].save({"network.module_0.bias": setup["torch"].zeros(3)}, bad)
    options.update({"mlamg_pnet_model": bad})
    with pytest.raises(RuntimeError, match="Could not load PNet model"):
        pre.MLAMG().initialize(_PC(setup["A"]))


def test_preconditioner_without_the_option_is_unchanged(setup, options):
    """No mlamg_pnet_model: P is bitwise the smoothed-aggregation P on Bellman-Ford aggregates."""
    import mlamg.preconditioner as pre
    import mlamg.problems
    from mlamg.hierarchy import Hierarchy
    A = mlamg.problems.poisson_2d_5pt(24)
    M = pre.MLAMG()
    M.initialize(_PC(A))
    assert M.pnet_model_fname == "" and not hasattr(M, "P_net")
    H = Hierarchy.build(A, alpha=0.1, max_levels=2, max_coarse=0, jacobi_weight=2.0 / 3.0,
                        finalize=False)
    want, got = H.levels[0].P.to_scipy(), M.H.levels[0].P.to_scipy()
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64))
