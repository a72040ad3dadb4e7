"""CPU: the float64 numpy references of the GNN kernels (oracle/gnn_kernels_ref.py) against the
torch restatement (oracle/gnn_ref.py functions / torch.nn.functional) for every case of
tests/test_gpu_gnn_kernels.py (lists in oracle/gnn_kernel_cases.py). The restatement with inputs
and weights cast to float64 must agree with the numpy reference to 1e-12 of the tensor's scale:
that validates the reference. The float32 run gives err_ref32, the error of a correct fp32
evaluation and the device tests' yardstick (printed here per case). The conditioning caps of the
generated inputs, the features the test graphs must have, and the sensitivity of the directed
cases to a src/tgt swap are asserted here too, so that whether a case list is admissible is decided
on the CPU and not by the kernel under test. No device call."""
import numpy as np
import pytest

pytest.importorskip("torch")

from oracle import gnn_kernel_cases as gc  # noqa: E402
from oracle import gnn_kernels_ref as kref  # noqa: E402

LISTS = {"linear": gc.linear_cases, "gcn_norm": gc.gcn_norm_cases,
         "propagate": gc.propagate_cases, "instance_norm": gc.instance_norm_cases,
         "nnconv": gc.nnconv_cases, "edge_mlp": gc.edge_mlp_cases}
SMALL_T = 4101  # the grid-cap cases' generators at a size the CPU checks in no time


def _check_fp64(c):
    """restate(float64) == ref64 to 1e-12 of the scale, for every tensor of the case."""
    r64, t64 = gc.ref64(c), gc.restate(c, "float64")
    yard = gc.yardsticks(c)
    for name in r64:
        for (label, ref, _), (_, got, _) in zip(gc.parts(c, name, r64[name]),
                                                gc.parts(c, name, t64[name])):
            _, err32, scale, tol = yard[label]
            assert got.dtype == np.float64 and np.all(np.isfinite(ref)), (c["id"], label)
            err = np.abs(got.reshape(ref.shape) - ref).max() if ref.size else 0.0
            print(f"{c['kernel']} {c['id']} {label}: |torch64 - ref64| / scale = "
                  f"{err / max(scale, 1e-300):.2e}, err_ref32 / scale = "
                  f"{err32 / max(scale, 1e-300):.2e}")
            assert err <= 1e-12 * scale, (c["id"], label, err, scale)
            assert tol >= 4 * gc.F32_EPS * scale


@pytest.mark.parametrize("kernel", sorted(LISTS))
def test_reference_matches_torch_in_float64(kernel):
    cases = LISTS[kernel]()
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        _check_fp64(c)


@pytest.mark.parametrize("kernel", ("propagate", "nnconv", "edge_mlp"))
def test_gridcap_generators_match_torch_in_float64(kernel):
    """The grid-cap cases use the same reference functions and the same generator at
    T = 4 * 2^20 + 5; the generator is checked here at a small T (its LayerNorm cap at the full T
    is in test_conditioning_caps), the full size is evaluated once, by the device test."""
    _check_fp64(gc.gridcap_case(kernel, SMALL_T))


def test_case_lists_cover_what_they_must():
    for shape in gc.LINEAR_SHAPES:
        mine = [c for c in gc.linear_cases() if (c["M"], c["K"], c["N"]) == shape]
        assert {c["b"] is None for c in mine} == {True, False}
        assert {c["act"] for c in mine} == {0, 1} and {c["beta"] for c in mine} == {0.0, 1.0}
        rcs = {None if c["R"] is None else c["R"].shape[1] for c in mine}
        assert rcs == {None, 1, shape[2]}
        assert all((c["Y0"] is not None) == (c["beta"] != 0) for c in mine)
    assert 20 <= len(gc.linear_cases()) <= 30
    for cases in (gc.nnconv_cases(), gc.edge_mlp_cases()):
        assert {c["act"] for c in cases} == {0, 1}
        rcs = set()  # residual kinds at outputs wider than 1 (where rc = 1 and rc = width differ)
        for c in cases:
            width = c["Fout"] if c["kernel"] == "nnconv" else c["C"]
            if c["R"] is None:
                rcs.add("none")
            elif width > 1:
                rcs.add("rc1" if c["R"].shape[1] == 1 else "full")
        assert rcs == {"none", "rc1", "full"}
    nn_shapes = {(c["graph"].n, c["Fin"], c["Fout"], c["fe"]) for c in gc.nnconv_cases()}
    assert {(301,) + s for s in gc.NNCONV_SHAPES} <= nn_shapes
    assert {(7,) + s for s in gc.NNCONV_SHAPES[:3]} <= nn_shapes
    em = {(c["graph"].n, c["F"], c["fe"], c["H"], c["C"]) for c in gc.edge_mlp_cases()}
    assert em == {(n,) + s for n in (301, 7) for s in gc.EDGE_MLP_SHAPES}
    assert {(c["n"], c["F"]) for c in gc.instance_norm_cases()} == \
        {(n, F) for n in gc.INORM_N for F in gc.INORM_F}
    ids = {c["id"] for c in gc.topk_cases()}
    assert "signed_zero-pair-k1" in ids and "ties-n6-k1" in ids
    for kind in gc.TOPK_KINDS:
        for n in gc.TOPK_N:
            if kind == "ties" and n != 6:
                continue
            for k in (0, 1, n // 10, n):
                assert f"{kind}-n{n}-k{k}" in ids


def test_graphs_have_the_required_features():
    g = gc.dir7()
    indeg, outdeg = np.bincount(g.tgt, minlength=7), np.bincount(g.src, minlength=7)
    assert g.n == 7 and indeg[0] == 0 and outdeg[0] > 0 and outdeg[6] == 0 and indeg[6] > 0
    assert [int(s) for s, t in zip(g.src, g.tgt) if t == 3] == [3]
    pairs = {(int(s), int(t)): float(w) for s, t, w in zip(g.src, g.tgt, g.w)}
    assert any((t, s) not in pairs for (s, t) in pairs if s != t), "pattern must be non-symmetric"
    assert any((t, s) in pairs and pairs[(t, s)] != w for (s, t), w in pairs.items() if s != t)
    assert np.all(g.w > 0) and len(g.w) - len(set(g.w.tolist())) == 1, "one duplicated weight"
    r = gc.ragged301()
    indeg = np.bincount(r.tgt, minlength=r.n)
    assert r.n == 301 and indeg.min() == 0 and indeg.max() == 40
    assert r.E % 64 != 0 and r.E % 4 != 0 and r.n % 4 != 0
    assert (r.src == r.tgt).sum() > 10 and r.w.min() >= 0.1 and r.w.max() <= 2.0
    assert len(set(zip(r.src.tolist(), r.tgt.tolist()))) == r.E, "no duplicate edges"
    mat = set(zip(r.src.tolist(), r.tgt.tolist()))
    assert sum((t, s) not in mat for s, t in mat) > r.E // 2, "directed"
    for gr in (g, r):  # tptr / teid: each target's incoming edges, ascending source
        for j in range(gr.n):
            e = gr.teid[gr.tptr[j]:gr.tptr[j + 1]]
            assert np.all(gr.tgt[e] == j) and np.all(np.diff(gr.src[e]) > 0)
        assert gr.tptr[-1] == gr.E
    e5 = gc.empty5()
    assert e5.n == 5 and e5.E == 0 and np.all(e5.tptr == 0)
    ring = gc.ring(SMALL_T)
    assert np.all(ring.tgt[ring.teid] == np.arange(SMALL_T)) and ring.tptr[-1] == SMALL_T
    assert np.all(np.bincount(ring.tgt) == 1) and len(np.unique(ring.w)) > SMALL_T // 2
    assert gc.T_CAP == 4 * 2 ** 20 + 5


def test_conditioning_caps():
    for c in gc.instance_norm_cases():
        X = c["X"].astype(np.float64)
        free = ~c["const"]
        assert np.all(X[:, c["const"]] == X[:1, c["const"]]), c["id"]
        if free.any():
            mean, std = X[:, free].mean(axis=0), X[:, free].std(axis=0)
            assert np.all(std > 0) and np.all(np.abs(mean) <= 10 * std), c["id"]
        if c["n"] > 1 and c["F"] >= 3:
            assert np.all(c["X"][:, -1] == np.float32(1.0 / c["n"]))
    reached = 0.0
    for c in gc.instance_norm_cases():
        if (~c["const"]).any():
            X = c["X"][:, ~c["const"]].astype(np.float64)
            reached = max(reached, float((np.abs(X.mean(axis=0)) / X.std(axis=0)).max()))
    assert reached > 8, "offsets should come close to the cap"
    for c in gc.edge_mlp_cases() + [gc.gridcap_case("edge_mlp")]:
        if c["H"] < 2:
            continue
        g = c["graph"]
        W1, b1 = c["W1"].astype(np.float64), c["b1"].astype(np.float64)
        X = c["X"].astype(np.float64)
        worst = 0.0
        for lo in range(0, g.E, 1 << 18):
            s, t = g.src[lo:lo + (1 << 18)], g.tgt[lo:lo + (1 << 18)]
            z = np.concatenate([X[s], X[t], c["ea"][lo:lo + (1 << 18)].astype(np.float64)], 1)
            h = np.maximum(z @ W1.T + b1, 0.0)
            worst = max(worst, float((np.abs(h.mean(axis=1)) /
                                      np.sqrt(h.var(axis=1) + 1e-5)).max()))
        assert worst <= 10, (c["id"], worst)


def test_directed_cases_tell_src_from_tgt():
    """A kernel that read the edges backwards must fail the dir7 (and ragged301) cases: the
    reference on the reversed graph is more than 100 tolerances away from the true one."""
    for c in gc.gcn_norm_cases() + gc.propagate_cases():
        g = c["graph"]
        if g.E == 0:
            continue
        yard = gc.yardsticks(c)
        rev = gc.ref64(dict(c, graph=gc.swapped(g)))
        for name, (ref, _, _, tol) in yard.items():
            diff = np.abs(rev[name].reshape(ref.shape) - ref).max()
            assert diff > 100 * tol, (c["id"], name, diff, tol)


def test_exact_properties_of_the_references():
    # nodes without incoming edges: dis == 0 and a zero propagated row, exactly
    for c in gc.gcn_norm_cases():
        g = c["graph"]
        lone = np.bincount(g.tgt, minlength=g.n) == 0
        assert lone.any() and np.all(gc.ref64(c)["dis"][lone] == 0.0)
    for c in gc.propagate_cases():
        g = c["graph"]
        assert np.all(gc.ref64(c)["Y"][np.bincount(g.tgt, minlength=g.n) == 0] == 0.0)
    # E == 0: NNConv is act(root + bias) (+ R)
    for c in gc.nnconv_cases():
        if c["graph"].E == 0:
            y = c["root"].astype(np.float64) + c["bias"].astype(np.float64)
            y = np.maximum(y, 0.0) if c["act"] else y
            y = y if c["R"] is None else y + c["R"]
            assert np.array_equal(gc.ref64(c)["Y"], y)
    # H == 1: LayerNorm of one value is its beta
    seen = 0
    for c in gc.edge_mlp_cases():
        if c["H"] == 1:
            y = c["W2"].astype(np.float64) @ c["beta"].astype(np.float64) + c["b2"]
            y = np.maximum(y, 0.0) if c["act"] else y
            y = np.broadcast_to(y, (c["graph"].E, c["C"]))
            y = y if c["R"] is None else y + c["R"]
            assert np.array_equal(gc.ref64(c)["out"], y)
            seen += 1
    assert seen == 2
    # a constant channel normalises to exactly 0
    for c in gc.instance_norm_cases():
        assert np.all(gc.ref64(c)["Y"][:, c["const"]] == 0.0)


def test_topk_reference_is_the_stable_sort():
    """kref.topk against gnn_ref.topk_vec / torch's stable descending sort, bitwise. NaN scores
    are left out: argsort and torch.sort leave their order to the implementation."""
    for c in gc.topk_cases():
        assert not np.isnan(c["scores"]).any()
        vec, idx = kref.topk(c["scores"], c["k"])
        tvec, tidx = gc.restate_topk(c["scores"], c["k"])
        assert vec.dtype == np.float32 and idx.dtype == np.int32
        assert np.array_equal(vec, tvec) and np.array_equal(idx, tidx), c["id"]
        assert int(vec.sum()) == c["k"] == len(idx)
    vec, idx = kref.topk(np.array([-0.0, 0.0], dtype=np.float32), 1)
    assert idx.tolist() == [0] and vec.tolist() == [1.0, 0.0]
    vec, idx = kref.topk(np.array([1.0, 3.0, 3.0, 0.0, 3.0, -1.0], dtype=np.float32), 3)
    assert idx.tolist() == [1, 2, 4]
    s = gc.topk_scores("signed_zero", 257)
    assert np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any()
    z = gc.topk_scores("relu70", 5000)
    assert 0.65 < (z == 0).mean() < 0.75
    assert np.isposinf(gc.topk_scores("inf", 257)).any()
    assert np.isneginf(gc.topk_scores("inf", 257)).any()
