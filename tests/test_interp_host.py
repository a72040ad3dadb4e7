"""CPU: the host-side pieces of mlamg.interp (the learned interpolation of ns/model/ali_interp.py)
and the yardstick the GPU tests hold its kernels to.

 - tests/interp_ref.py, the plain-torch restatement of ResidualBlock / EdgeModel / forward, gives
   the same network in float32 and float64 to float32 accuracy at seeded weights;
 - assemble_P on CPU tensors is bitwise the reference's scipy assembly, for a C in non-ascending
   order;
 - graph_from_matrix keeps exactly the C-F edges;
 - the modules' state_dict carries every documented key and round-trips."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import greedy_cases as gc
import interp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "greedy_cf.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def problem(golden):
    """The 12 x 12 grid with the reference's splitting at theta 0.56 (50 coarse points), its C-F
    graph on the CPU and a seeded network."""
    from mlamg import interp
    A = gc.poisson_2d(12)
    C, F = golden["grid_12_C"], golden["grid_12_F"]
    g = interp.graph_from_matrix(A, C, F, device="cpu")
    net = interp.InterpolationNetwork()
    sd = interp_ref.seeded_state_dict(net.model, 2024)
    return A, C, F, g, net, sd


def test_graph_keeps_exactly_the_cf_edges(problem):
    from mlamg import interp
    A, C, F, g, _, _ = problem
    n = A.shape[0]
    src, tgt = g.src.numpy(), g.tgt.numpy()
    is_c = np.zeros(n, dtype=bool)
    is_c[C] = True
    assert np.all(is_c[src] != is_c[tgt]) and np.all(src != tgt)
    # every stored C-F entry of A, row-major, both directions
    coo = A.tocoo()
    keep = is_c[coo.row] != is_c[coo.col]
    assert np.array_equal(src, coo.row[keep]) and np.array_equal(tgt, coo.col[keep])
    pairs = set(zip(src.tolist(), tgt.tolist()))
    assert all((t, s) in pairs for s, t in pairs)
    assert np.array_equal(g.edge_attr.numpy()[:, 0], np.abs(coo.data[keep]).astype(np.float32))
    assert np.array_equal(g.x.numpy()[:, 0], is_c.astype(np.float32))
    B = A.tolil()
    B[0, 1] = -3.0
    with pytest.raises(ValueError, match="symmetric"):
        interp.graph_from_matrix(B.tocsr(), C, F, device="cpu")
    with pytest.raises(ValueError, match="split"):
        interp.graph_from_matrix(A, C, F[:-1], device="cpu")


def test_assemble_P_is_the_scipy_assembly(problem):
    from mlamg import interp
    A, C, F, g, _, _ = problem
    n = A.shape[0]
    C = np.asarray(C)[::-1].copy()  # descending: non-ascending whatever the golden order
    assert np.any(np.diff(C) < 0)
    vals = torch.rand(g.E, 1, generator=torch.Generator().manual_seed(3)) + 0.25
    indptr, indices, data = interp.assemble_P(n, g.src, g.tgt, vals, C)
    ref = interp_ref.scipy_P(n, g.src.numpy(), g.tgt.numpy(), vals.numpy(), C)
    ref.sort_indices()
    assert ref.shape == (n, len(C)) and ref.dtype == np.float32
    assert np.array_equal(indptr.numpy(), ref.indptr)
    assert np.array_equal(indices.numpy(), ref.indices)
    assert data.dtype == torch.float64
    assert np.array_equal(data.numpy(), ref.data.astype(np.float64))
    # unit rows on C, in C's column order
    P = sp.csr_matrix((data.numpy(), indices.numpy(), indptr.numpy()), shape=(n, len(C)))
    for col, c in enumerate(C):
        row = P.getrow(c)
        assert row.nnz == 1 and row.indices[0] == col and row.data[0] == 1.0


def test_state_dict_keys_and_round_trip(problem):
    from mlamg import interp
    _, _, _, _, net, sd = problem
    keys = set(sd)
    dims = interp_ref.DIMS
    for pos in [p for blk in interp_ref.NODE_BLOCKS for p in blk]:
        for k in range(interp_ref.HOPS + 1):
            assert f"network.module_{pos}.lins.{k}.weight" in keys
        assert f"network.module_{pos}.bias" in keys
    assert sd["network.module_0.lins.0.weight"].shape == (dims[0], 1)
    assert sd["network.module_28.lins.5.weight"].shape == (256, 256)
    lin_pos = [0] + [p for i in range(9) for p in (1 + 3 * i, 3 + 3 * i)] + [28]
    for j in lin_pos:
        assert f"edge_model.network.{j}.weight" in keys and f"edge_model.network.{j}.bias" in keys
    for i in range(interp_ref.N_EDGE_BLOCKS):
        for j in ((0,) if i in (0, 10) else (0, 2)):
            assert f"edge_model.blocks.{i}.{j}.weight" in keys
            assert f"edge_model.blocks.{i}.{j}.bias" in keys
        if i < 10:
            assert f"edge_model.normaliz.{i}.weight" in keys
    assert sd["edge_model.blocks.0.0.weight"].shape == (256, 513)
    assert sd["edge_model.blocks.10.0.weight"].shape == (1, 16)
    # blocks and network hold the same tensors, like the reference's
    assert sd["edge_model.blocks.1.2.weight"].data_ptr() == sd["edge_model.network.3.weight"].data_ptr()
    other = interp.InterpolationNetwork()
    missing, unexpected = other.model.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert not missing and not unexpected
    for k, v in other.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert sum(p.numel() for p in net.parameters()) == sum(
        v.numel() for k, v in sd.items() if not k.startswith("edge_model.network."))


def test_restatement_float32_agrees_with_float64(problem):
    """The yardstick itself: its float32 evaluation (both orders) lies within float32 accuracy of
    its float64 one. The bound is 2^-24 * 31 * 64 * gain * scale: the network is 31 normalised
    blocks deep, a block commits up to 64 roundings of 2^-24 relative to its O(1) activations
    (six 256-term products, propagations, normalisation), and `gain` is how strongly the float64
    network itself answers a perturbation of that size: every parameter is multiplied by
    1 +- 2^-24 (seeded signs) and the float64 output's change, in units of 2^-24 * scale, is the
    gain (at least 1). The gain is a property of the function (the InstanceNorms and the final
    division by the standard deviation amplify), not of any float32 code. A wrong layer is off by
    O(1), thousands of bounds."""
    _, _, _, g, _, sd = problem
    src, tgt, ea = g.src.numpy(), g.tgt.numpy(), g.edge_attr.numpy()[:, 0]
    x0 = g.x.numpy()
    x64, e64 = interp_ref.Ref(sd, src, tgt, ea, torch.float64).forward(x0)
    assert torch.isfinite(e64).all() and e64.shape == (g.E, 1) and float(e64.std()) > 0.1
    gen = torch.Generator().manual_seed(5)
    bumped = {k: v.double() * (1 + 2.0 ** -24 * (2 * torch.randint(0, 2, v.shape, generator=gen)
                                                 - 1)) for k, v in sd.items()}
    xb, eb = interp_ref.Ref(bumped, src, tgt, ea, torch.float64).forward(x0)
    unit = 2.0 ** -24
    gains = {"nodes": max(1.0, float((xb - x64).abs().max()) / (unit * float(x64.abs().max()))),
             "edges": max(1.0, float((eb - e64).abs().max()) / (unit * float(e64.abs().max())))}
    print(f"[interp-ref] gains {gains}")
    for rev in (False, True):
        x32, e32 = interp_ref.Ref(sd, src, tgt, ea, torch.float32, reverse=rev).forward(x0)
        for name, a, b in (("nodes", x32, x64), ("edges", e32, e64)):
            err = float((a.double() - b).abs().max())
            scale = float(b.abs().max())
            print(f"[interp-ref] reverse={rev} {name}: err/scale {err / scale:.3e} "
                  f"bound/scale {unit * 31 * 64 * gains[name]:.3e}")
            assert err <= unit * 31 * 64 * gains[name] * scale, (rev, name, err, scale)
    # the reversed order is the same function
    x64r, e64r = interp_ref.Ref(sd, src, tgt, ea, torch.float64, reverse=True).forward(x0)
    assert float((e64r - e64).abs().max()) <= 1e-9 * float(e64.abs().max())
